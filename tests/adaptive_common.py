"""What the adaptive-sampling tests share (test_adaptive_ref.py, test_gpu_adaptive.py): the oracle's
samples of a case, computed once -- helpers only, no tests and no fixtures."""
import functools

import numpy as np

import oracle
from opengl_ray_tracing_amd import orbit_camera, scenes

F = np.float32
FRAMES = 32
EVERY = 8
PRM = dict(threshold=4 / 255, limit=1.5, min_frames=8)
# name -> (scene config, integrator (None: the config's), max_bounce (None: the config's))
CASES = {"c2": ("c2", None, None), "c3": ("c3", None, None), "c4": ("c4", None, None),
         "c3-disney": ("c3", "disney", -1)}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (integrator, max_bounce, tris, nodes, hdr, eye, rot) of a case above."""
    scene, integ, mb = CASES[name]
    cfg, tris, nodes, hdr = scenes.build_config(scene)
    eye, rot = orbit_camera(*cfg.camera)
    return (cfg.integrator if integ is None else integ, cfg.max_bounce if mb is None else mb, tris, nodes, hdr,
            eye, rot)


@functools.lru_cache(maxsize=None)
def the_oracle(name):
    _, _, tris, nodes, hdr, _, _ = case(name)
    return oracle.Oracle(tris, nodes, hdr)


@functools.lru_cache(maxsize=None)
def samples(name, w, h):
    """The oracle's FRAMES samples of a case, kept per sample (sample k alone: frame 0 of sample rank k
    of FRAMES, so its weight is 1 and its sample index k, as test_gpu_variance.oracle_moments does):
    a tuple of read-only (h, w, 4) planes, computed once per case."""
    integ, mb, _, _, _, eye, rot = case(name)
    orc = the_oracle(name)
    out = []
    for k in range(FRAMES):
        s, _ = orc.render(w, h, integ, 0, eye, rot, accum=np.zeros((h, w, 4), F), max_bounce=mb, sample_rank=k,
                          sample_world=FRAMES)
        s.setflags(write=False)
        out.append(s)
    return tuple(out)
