"""The row pruning of phase B (lsc_planner_amd/csrc/lsc_kernels.hip, `unit_rows`; second copy in lsc_general.hpp), restated once in
float64 numpy from the reference's rows and DESIGN section 4.1 -- not from the kernels.

The reference's QP (src/traj_optimizer.cpp) holds, per axis and with n = 5, the velocity rows |c_{j+1} - c_j| <= V = vmax dt / n and the
acceleration rows |c_{j+2} - 2 c_{j+1} + c_j| <= A = amax dt^2 / (n (n - 1)) inside every segment, and joins segments C0 .. C2: the last
point of a segment is the first of the next, and the last first and second differences of a segment are the first ones of the next.
c_{0,0}, c_{0,1}, c_{0,2} are fixed by the current state.  Walk the control points from c_{0,2}: c_{m,i} is reached after K = 5 m + i - 2
steps (c_{m,5} and c_{m+1,0} are one point), the first step d0 = c_{0,2} - c_{0,1} is known, every step lies in [-V, V], and consecutive
steps differ by at most A.  Hence step j lies in [max(-V, d0 - j A), min(V, d0 + j A)] and

    lo[K] = sum_{j<=K} (max(-V, d0 - j A) - pad)  <=  c_{m,i} - c_{0,2}  <=  sum_{j<=K} (min(V, d0 + j A) + pad) = hi[K]

(pad = 1e-9 per step, the project's allowance for its own rounding).  An LSC row n . c_{m,i} >= rhs, rhs = d_{m,i} + n . q_{m,i} (q the
obstacle's predicted control point, d the margin), is dropped when the smallest n . c over that box still satisfies it with 1e-6 to spare:

    worst = n . c_{0,2} + sum_k n_k (n_k >= 0 ? lo_k[K] : hi_k[K])  >=  rhs + 1e-6.

(The bound is loose by one step per segment end: the step that C1 duplicates is counted twice.)  That the box holds every point of the
reference's polytope, and that every dropped row is redundant there, is what tests/test_prune_soundness.py proves by LP.

    reach_bounds    lo[K], hi[K], K = 0 .. 27
    kept_rows       one agent against all its obstacles: which rows stay, how far each is from the threshold, counts per control point
    count_band      what a kernel's row count and fullest bucket may be, given the rows within `band` of the threshold
    general_count   the count lsc_general_kernel reports: kept rows + its group sign rows
"""
import numpy as np

NC, DEG = 6, 5
PAD_STEP = 1e-9          # per step of the box
PAD_ROW = 1e-6           # on the row's right-hand side
BAND = 1e-9              # a row this close to the threshold may fall either way in another order of additions


def limits(max_vel, max_acc, dt):
    """(V, A): the largest step between consecutive control points and the largest change of that step, per axis."""
    return np.asarray(max_vel, np.float64) * (dt / DEG), np.asarray(max_acc, np.float64) * (dt * dt / (DEG * (DEG - 1)))


def reach_bounds(d0, V, A, pad=PAD_STEP, steps=27):
    """(lo, hi), each [..., steps + 1]: bounds of c - c_{0,2} after K = 0 .. steps steps along one axis (broadcast over the leading
    shape); lo[0] = hi[0] = 0."""
    d0, V, A = (np.asarray(x, np.float64)[..., None] for x in np.broadcast_arrays(d0, V, A))
    j = np.arange(1, steps + 1, dtype=np.float64)
    lo = np.cumsum(np.maximum(-V, d0 - j * A) - pad, axis=-1)
    hi = np.cumsum(np.minimum(V, d0 + j * A) + pad, axis=-1)
    z = np.zeros(lo.shape[:-1] + (1,))
    return np.concatenate([z, lo], axis=-1), np.concatenate([z, hi], axis=-1)


def steps_of(M):
    """K [M][6] = 5 m + i - 2: steps from c_{0,2} to c_{m,i} (<= 0: fixed by the state, no row)."""
    return DEG * np.arange(M)[:, None] + np.arange(NC)[None, :] - 2


def kept_rows(c02, d0, V, A, points, normal, d, planar=False, prune=1, ncs=None, mutate=None):
    """One agent against its n_obs obstacles.  c02, d0, V, A [3]; points [n_obs][M][6][3] the obstacles' predicted control points;
    normal [n_obs][M][3]; d [n_obs][M][6] the margins.  planar: the row has no z term.  prune: 0 keeps every candidate row (27 per
    obstacle at M = 5), 1 and 3 apply the rule, 2 the velocity-only formula worst = n . c_{0,2} - K sum_k |n_k| V_k.  ncs: the general
    kernel builds rows of segments m < ncs only (None: all).  mutate: a deliberately wrong rule, for showing that a check can see one --
    dict(shift=s) takes the box s steps off (K + s), dict(swap=True) takes hi where lo belongs, dict(pad=-1) flips the per-step pad.
    Returns (keep bool [n_obs][M][6], gap float [n_obs][M][6] = worst - (rhs + 1e-6), +inf where there is no candidate row,
    counts int [6 M] kept rows per control point)."""
    mutate = mutate or {}
    points, d = np.asarray(points, np.float64), np.asarray(d, np.float64)
    n = np.array(normal, np.float64)
    M = n.shape[1]
    if planar:
        n[..., 2] = 0.0
    c02, d0, V, A = (np.asarray(x, np.float64).reshape(3) for x in (c02, d0, V, A))
    K = steps_of(M)
    cand = np.broadcast_to((K >= 1) & (np.arange(M)[:, None] < (M if ncs is None or ncs < 0 else min(ncs, M))), d.shape)
    rhs = d + (n[:, :, None, :] * points).sum(axis=-1)
    centre = n @ c02                                                         # [n_obs][M]
    if prune == 2:
        worst = centre[:, :, None] - K[None] * (np.abs(n) @ V)[:, :, None]
    else:
        lo, hi = reach_bounds(d0, V, A, pad=PAD_STEP * mutate.get("pad", 1))                 # [3][28]
        if mutate.get("swap"):
            lo, hi = hi, lo
        Ks = np.clip(K + mutate.get("shift", 0), 0, lo.shape[-1] - 1)
        box = np.where(n[:, :, None, :] >= 0.0, lo[:, Ks].transpose(1, 2, 0)[None], hi[:, Ks].transpose(1, 2, 0)[None])      # [n_obs][M][6][3]
        worst = centre[:, :, None] + (n[:, :, None, :] * box).sum(axis=-1)
    gap = np.where(cand, worst - (rhs + PAD_ROW), np.inf)
    keep = cand & (gap < 0.0) if prune else cand.copy()
    return keep, gap, keep.reshape(len(keep), -1).sum(axis=0)


def count_band(keep, gap, prune=1, band=BAND):
    """What a correct kernel may report: (count_lo, count_hi, bucket_max_lo, bucket_max_hi).  Rows with |gap| <= band are borderline:
    count_lo holds the rows kept for sure, count_hi those and the borderline ones.  (prune = 0: no row is borderline.)"""
    flat_keep, flat_gap = keep.reshape(len(keep), -1), gap.reshape(len(gap), -1)
    edge = (np.abs(flat_gap) <= band) if prune else np.zeros_like(flat_keep)
    sure = flat_keep & ~edge
    lo_b, hi_b = sure.sum(axis=0), (sure | edge).sum(axis=0)
    return int(lo_b.sum()), int(hi_b.sum()), int(lo_b.max(initial=0)), int(hi_b.max(initial=0))


def general_count(keep, slack):
    """Rows lsc_general_kernel counts: the kept collision rows, and for every obstacle that carries slack variables (slack bool [n_obs])
    one sign row e >= 0 per segment group with a kept row (the group's slack variable exists only then)."""
    slack = np.asarray(slack, bool)
    return int(keep.sum() + keep.any(axis=2)[slack].sum())
