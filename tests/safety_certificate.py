"""Continuous-time separation certificate of a tick's plans, from the output alone (plain numpy, float64; no oracle, no product import).

For a pair (i, j) and a segment m both curves are degree-5 Bernstein polynomials over the same interval, so their difference at any t is a
convex combination -- with the Bernstein weights -- of the six index-matched differences c_i[m][k] - c_j[m][k].  With z divided by the
pair's downwash (dw_i r_i + dw_j r_j) / (r_i + r_j) (generateLSC, src/traj_planner.cpp:1339-1345) the pair collides at no instant of the
segment if the distance from the origin to the convex hull of those six points is at least r_i + r_j.  Both LSC and BVC promise exactly
this to two agents that both solved their QP: agent i's row n . (c_i[k] - o_j[k]) >= d_i[k] and agent j's row against i, summed, are
n . (c_i[k] - c_j[k]) >= r_i + r_j for every k.

hull_distance does not iterate (no GJK): it projects the origin onto the affine span of every face of 1 to 4 vertices (56 subsets), keeps
the projections whose barycentric weights are all >= 0 and takes the nearest.  The closest point of the hull is the projection onto the
span of the vertices that carry it (Caratheodory: at most 4, affinely independent), so it is among the candidates; every candidate is
evaluated as the weighted sum of its vertices and is therefore a point of the hull whatever a degenerate subset's solve returned, so no
candidate is nearer than the hull.

Out of scope (the tests that use this module certify none of these):
  - slack modes (dynamical_limit, collision_constraint): their rows may be violated by design;
  - agents after a disturbance reset: their initial trajectory is not the plan their neighbours built rows against;
  - dynamic obstacles: the agent takes half of the separation from an obstacle that takes none -- the reference
    promises nothing there;
  - goal planning: it moves goals, not plans; a plan towards any goal carries the same rows.
"""
from itertools import combinations

import numpy as np

NC = 6                                              # control points of a segment (degree 5)
BOX_CLEARANCE = 0.01                                # metres; see pair_certificate
_FACES = {k: np.array(list(combinations(range(NC), k))) for k in (1, 2, 3, 4)}      # 6 + 15 + 20 + 15 = 56 subsets


def hull_distance(P):
    """Distance from the origin to conv(P[..., 6, 3]), float64, vectorised over the leading axes."""
    P = np.asarray(P, np.float64)
    assert P.shape[-2:] == (NC, 3), P.shape
    flat = P.reshape(-1, NC, 3)
    best = np.linalg.norm(flat, axis=2).min(axis=1)                     # the 6 vertices
    dot = lambda a, b: (a * b).sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):                # a degenerate face divides by 0: its weights fail w >= 0 or are sound
        for k in (2, 3, 4):
            V = flat[:, _FACES[k], :]                                   # [B][S][k][3]
            v0 = V[:, :, 0, :]
            a = [V[:, :, i, :] - v0 for i in range(1, k)]               # the edges from the first vertex
            # weights lam of the edges at the projection of the origin onto v0 + span(a): the normal equations, solved in closed form
            if k == 2:
                lam = [-dot(a[0], v0) / dot(a[0], a[0])]
            elif k == 3:
                g00, g01, g11, b0, b1 = dot(a[0], a[0]), dot(a[0], a[1]), dot(a[1], a[1]), -dot(a[0], v0), -dot(a[1], v0)
                det = g00 * g11 - g01 * g01
                lam = [(g11 * b0 - g01 * b1) / det, (g00 * b1 - g01 * b0) / det]
            else:                                                       # a tetrahedron spans the space: the projection is the origin itself
                c12, c20, c01 = np.cross(a[1], a[2]), np.cross(a[2], a[0]), np.cross(a[0], a[1])
                det = dot(a[0], c12)
                lam = [-dot(v0, c12) / det, -dot(v0, c20) / det, -dot(v0, c01) / det]
            w = np.stack([1.0 - sum(lam)] + lam, axis=-1)
            x = (w[..., None] * V).sum(axis=-2)                         # a point of the hull whenever w >= 0: the weights sum to 1
            d = np.where((w >= 0.0).all(axis=-1), np.linalg.norm(x, axis=-1), np.inf)
            best = np.minimum(best, d.min(axis=1))
    return best.reshape(P.shape[:-2])


def pair_downwash(r_i, dw_i, r_j, dw_j):
    return (dw_i * r_i + dw_j * r_j) / (r_i + r_j)


def control_points(traj, M):
    """[N][3][M * 6] (or flattened) -> float64 [N][M][6][3]."""
    t = np.asarray(traj, np.float64)
    return np.moveaxis(t.reshape(len(t), 3, M, NC), 1, 3)


class Certificate:
    """margin [pairs][M]: dist - (r_i + r_j) of pair (i[p], j[p]) in segment m, a masked array -- masked where either agent's status is not
    0; worst / where = (i, j, m): the smallest unmasked margin; excluded_agents / excluded_pairs: what the mask covers; boxed: the
    (pair, segment)s certified by their bounding boxes alone, whose margin is the boxes' (a lower bound of the hull's)."""

    def __init__(self, i, j, margin, excluded_agents, boxed):
        self.i, self.j, self.margin, self.excluded_agents, self.boxed = i, j, margin, int(excluded_agents), int(boxed)
        self.excluded_pairs = int(np.ma.getmaskarray(margin)[:, 0].sum()) if margin.size else 0
        if margin.count():
            p, m = np.unravel_index(int(np.ma.argmin(margin)), margin.shape)
            self.worst, self.where = float(margin[p, m]), (int(i[p]), int(j[p]), int(m))
        else:
            self.worst, self.where = np.inf, None

    def of_pair(self, a, b):
        """Margins [M] of the pair {a, b}."""
        a, b = min(a, b), max(a, b)
        return self.margin[np.nonzero((self.i == a) & (self.j == b))[0][0]]


def pair_certificate(traj, radius, downwash, M, status=None, planar=False, prefilter=None, chunk=1 << 15):
    """The certificate of one tick's plans: traj [N][3][M * 6], radius and downwash [N].  planar: the hull is taken in x, y, as the
    reference's 2-D model holds z at world/z_2d for everybody.  prefilter (default: swarms of more than 16 agents): a (pair, segment)
    whose control points' axis-aligned boxes are more than r_i + r_j + BOX_CLEARANCE apart after the downwash scaling is certified by that
    alone -- each index-matched difference lies between the boxes' gaps, so the hull is at least as far --; every other one goes through
    hull_distance.  (The clearance keeps the boxes' lower bounds out of any count of pairs that nearly touch.)"""
    c = control_points(traj, M)
    N = len(c)
    r, dw = np.asarray(radius, np.float64), np.asarray(downwash, np.float64)
    ii, jj = np.triu_indices(N, 1)
    if prefilter is None:
        prefilter = N > 16
    lo, hi = c.min(axis=2), c.max(axis=2)                               # [N][M][3]
    margin = np.empty((len(ii), M))
    boxed = 0
    for s in range(0, len(ii), chunk):
        a, b = ii[s:s + chunk], jj[s:s + chunk]
        rsum = r[a] + r[b]
        scale = np.ones((len(a), 1, 3))
        scale[:, 0, 2] = 0.0 if planar else 1.0 / pair_downwash(r[a], dw[a], r[b], dw[b])
        out = np.empty((len(a), M))
        need = np.ones((len(a), M), bool)
        if prefilter:
            gap = np.maximum(0.0, np.maximum(lo[a] - hi[b], lo[b] - hi[a])) * scale
            box = np.linalg.norm(gap, axis=2)
            need = box <= rsum[:, None] + BOX_CLEARANCE
            out[~need] = (box - rsum[:, None])[~need]
            boxed += int((~need).sum())
        p, m = np.nonzero(need)
        if len(p):
            D = (c[a[p], m] - c[b[p], m]) * scale[p]                    # [K][6][3]
            out[p, m] = hull_distance(D) - rsum[p]
        margin[s:s + chunk] = out
    bad = np.zeros(N, bool) if status is None else (np.asarray(status) != 0)
    mask = np.repeat((bad[ii] | bad[jj])[:, None], M, axis=1)
    return Certificate(ii, jj, np.ma.array(margin, mask=mask), bad.sum(), boxed)


def starts_apart(start, radius, downwash):
    """The premise of the induction: smallest (downwash-scaled distance) - (r_i + r_j) over the pairs of starting points."""
    p, r, dw = np.asarray(start, np.float64), np.asarray(radius, np.float64), np.asarray(downwash, np.float64)
    ii, jj = np.triu_indices(len(p), 1)
    d = p[ii] - p[jj]
    d[:, 2] /= pair_downwash(r[ii], dw[ii], r[jj], dw[jj])
    return float((np.linalg.norm(d, axis=1) - (r[ii] + r[jj])).min())


def storage_bound(world_min, world_max, downwash):
    """Part (a) of the bound: what float32 storage of an exact plan can take from the certified distance.  A stored control point is
    within half an ulp of the exact one per coordinate, an ulp being that of the world's extent E_k = max(|min_k|, |max_k|) on the axis;
    a difference of two agents' points is then within one ulp(E_k) per axis, z after the division by the smallest pair downwash (a
    radius-weighted mean, so no smaller than the smallest agent's); the distance to a hull moves by no more than its vertices do."""
    E = np.maximum(np.abs(np.asarray(world_min, np.float32)), np.abs(np.asarray(world_max, np.float32)))
    ulp = np.spacing(E).astype(np.float64)
    ulp[2] /= float(np.min(downwash))
    return float(np.linalg.norm(ulp))
