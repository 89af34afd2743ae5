"""The specification of the ranged ray queries (include/pt_abi.h pt_trace_closest_range,
pt_trace_occluded and their device forms), stated against the unbounded query: with (t*, tri*) what
pt_trace_closest -- oracle.Oracle.trace_closest -- returns for a ray (a miss: 2147483648.0, -1) and b
the ray's bound,

    ranged closest: (t*, tri*) if tri* >= 0 and t* < b, else the miss values
    occluded:       1          if tri* >= 0 and t* < b, else 0

The comparison is strict, a NaN bound compares false (a miss), and since no accepted hit has
t* < 0.0005 (hitTriangle's lower bound) every b <= 0.0005 is a miss. No bound: every t* passes.
Helpers only: no tests and no fixtures."""
import numpy as np

F = np.float32
MISS_T = F(2147483648.0)
T_MIN = F(0.0005)  # hitTriangle rejects t < 0.0005 (pass1.fsh:251-301)

# the bounds every test applies to every ray, as functions of the ray's t*
BOUND_KINDS = ("t", "t_up", "t_down", "zero", "tmin", "minus_one", "inf", "nan")


def query_ref(t_star, tri_star, b=None):
    """-> (t, tri, occ): float32, int32, uint8 per ray."""
    t_star = np.ascontiguousarray(t_star, F).reshape(-1)
    tri_star = np.ascontiguousarray(tri_star, np.int32).reshape(-1)
    hit = tri_star >= 0
    if b is not None:
        b = np.ascontiguousarray(b, F).reshape(-1)
        with np.errstate(invalid="ignore"):
            hit = hit & (t_star < b)
    t = np.where(hit, t_star, MISS_T).astype(F)
    tri = np.where(hit, tri_star, -1).astype(np.int32)
    return t, tri, hit.astype(np.uint8)


def bound(kind: str, t_star) -> np.ndarray:
    """The bound of kind `kind` for every ray (t* of a miss is the miss value)."""
    t = np.ascontiguousarray(t_star, F).reshape(-1)
    if kind == "t":
        return t.copy()
    if kind == "t_up":
        return np.nextafter(t, F(np.inf)).astype(F)
    if kind == "t_down":
        return np.nextafter(t, F(-np.inf)).astype(F)
    const = {"zero": 0.0, "tmin": T_MIN, "minus_one": -1.0, "inf": np.inf, "nan": np.nan}[kind]
    return np.full(t.shape, const, F)


def mixed_bounds(t_star) -> np.ndarray:
    """Ray k with the bound of kind k % len(BOUND_KINDS): every kind side by side in one wave."""
    t = np.ascontiguousarray(t_star, F).reshape(-1)
    out = np.empty_like(t)
    for i, kind in enumerate(BOUND_KINDS):
        out[i::len(BOUND_KINDS)] = bound(kind, t)[i::len(BOUND_KINDS)]
    return out


def hemisphere_rays(P, N, k: int, seed: int) -> np.ndarray:
    """k seeded directions per point in the hemisphere about its normal, leaving the point itself:
    (len(P) * k, 6) float32, point-major."""
    P = np.ascontiguousarray(P, F).reshape(-1, 3)
    N = np.ascontiguousarray(N, F).reshape(-1, 3)
    rs = np.random.RandomState(seed)
    d = rs.normal(size=(P.shape[0], k, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    flip = np.einsum("pkc,pc->pk", d, N.astype(np.float64)) < 0
    d[flip] = -d[flip]
    rays = np.empty((P.shape[0], k, 6), F)
    rays[:, :, 0:3] = P[:, None, :]
    rays[:, :, 3:6] = d.astype(F)
    return rays.reshape(-1, 6)
