"""What the neighbour-list kernels (lsc_planner_amd/csrc/lsc_neigh.hip) have to compute, stated in float64 numpy from a tick's inputs -- no
GPU, no kernel arithmetic restated: tests/test_gpu_neighbour_lists.py holds SwarmPlanner.neighbour_dump() to these values.

    predicted_points   load_segment: the oracle's shift_traj / const_vel_traj of every agent
    cull_b             phase B's cullB[m] (lsc_kernels.hip: S.reachL / reachU by running sums, then max_i (|c_{0,2} - p_{m,i}| + |e_K|)) and the
                       build kernel's own bound in exact arithmetic
    unit_test_keeps    phase B's "spatial pre-cull" of one (obstacle, segment) unit; unit_test_keeps_all: the same for all units of an agent
    sphere_test        base and |D| of the query kernel's sphere test, from the dumped float32 spheres and reach
    priority_dist      rule_distf: float32 differences and products, the square root in double
"""
import numpy as np

from prune_reference import reach_bounds

NC, DEG = 6, 5
F = np.float32


def predicted_points(O, state, prev, planner_seq, dt, M):
    """float64 [N][M][6][3]: the control points every agent is predicted at (and plans from), as load_segment states them:
    oracle.const_vel_traj for planner_seq < 2, oracle.shift_traj of the previous plan otherwise."""
    state = np.ascontiguousarray(state, np.float32)
    prev = np.ascontiguousarray(prev, np.float32)
    N = len(state)
    out = np.zeros((N, 3, NC * M), np.float32)
    with O.segments(M):
        for q in range(N):
            out[q] = O.const_vel_traj(state[q, :3], state[q, 3:6], dt) if planner_seq < 2 else O.shift_traj(prev[q]).reshape(3, NC * M)
    return out.reshape(N, 3, M, NC).transpose(0, 2, 3, 1).astype(np.float64)


def state_constants(state, dt, planar=False, z2d=1.0):
    """(c_{0,2}, d0 = c_{0,2} - c_{0,1}) of every agent and axis in float64 from the float32 state (rule_state_constants)."""
    s = np.asarray(state, np.float32).astype(np.float64)
    hv, ha = dt / DEG, dt * dt / (DEG * (DEG - 1))
    c0 = s[:, 0:3]
    c1 = c0 + s[:, 3:6] * hv
    c2 = s[:, 6:9] * ha + 2.0 * c1 - c0
    if planar:
        c1, c2 = c1.copy(), c2.copy()
        c1[:, 2] = z2d
        c2[:, 2] = z2d
    return c2, c2 - c1


def reach_sums(d0, V, A):
    """e_K for K = 0..27 along one axis (broadcast over the leading shape): the larger magnitude of the running sums
    reachL[K] = sum_{j<=K} (max(-V, d0 - j A) - 1e-9), reachU[K] = sum_{j<=K} (min(V, d0 + j A) + 1e-9); e_0 = 0."""
    lo, hi = reach_bounds(d0, V, A)                   # (the sums are stated in tests/prune_reference.py)
    return np.maximum(np.abs(lo), np.abs(hi))


def cull_b(state, points, max_vel, max_acc, dt, planar=False, z2d=1.0):
    """(cullB [N][M], bound [N][M]).  cullB[m] = max_i (|c_{0,2} - p_{m,i}| + |e_K|) over K = 5 m + i - 2 >= 1 as phase B forms it;
    bound = (max_i |c_{0,2} - p_{m,i}| + max_i |e_K|) (1 + 1e-5) + 1e-3 + 1e-5 sum_k |c_{0,2}|: the build kernel's B_m in exact arithmetic."""
    N, M = points.shape[:2]
    c2, d0 = state_constants(state, dt, planar, z2d)
    V = np.asarray(max_vel, np.float64).reshape(N, 3) * (dt / DEG)
    A = np.asarray(max_acc, np.float64).reshape(N, 3) * (dt * dt / (DEG * (DEG - 1)))
    e = reach_sums(d0, V, A)                                                  # [N][3][28]
    K = DEG * np.arange(M)[:, None] + np.arange(NC)[None, :] - 2              # [M][6]
    has = K >= 1
    er = np.sqrt((e[:, :, np.maximum(K, 1)] ** 2).sum(axis=1))                # [N][M][6]
    dist = np.sqrt(((c2[:, None, None, :] - points) ** 2).sum(axis=-1))       # [N][M][6]
    dist, er = np.where(has, dist, 0.0), np.where(has, er, 0.0)
    cullB = (dist + er).max(axis=-1)
    bound = (dist.max(axis=-1) + er.max(axis=-1)) * (1.0 + 1e-5) + 1e-3 + 1e-5 * np.abs(c2).sum(axis=-1)[:, None]
    return cullB, bound


def pair_scale(r_a, dw_a, r_o, dw_o):
    """(1 / downwash of the pair, s = max(1, 1 / downwash)): the radius-weighted mean of generateLSC (traj_planner.cpp:1339-1345)."""
    idw = 1.0 / ((dw_a * r_a + np.asarray(dw_o, np.float64) * r_o) / (r_a + np.asarray(r_o, np.float64)))
    return idw, np.maximum(1.0, idw)


def unit_test_keeps(p, q, idw, B, r):
    """phase B's test on the six control points of both sides: keep unless |w_c| >= 2 s B + r + 2e-4 + R_w"""
    S = np.array([1.0, 1.0, idw])
    w = (p - q) * S
    wc = w.mean(axis=0)
    rw = np.sqrt(((w - wc) ** 2).sum(axis=1).max())
    need = 2.0 * max(1.0, idw) * B + r + 2e-4 + rw
    return not (wc @ wc >= need * need)


def unit_test_keeps_all(p, Q, idw, B, r):
    """unit_test_keeps for every unit of one agent: p [M][6][3] its points, Q [N][M][6][3] everybody's, idw [N], r [N] per pair,
    B [M] its cullB.  bool [N][M] (the agent's own row means nothing)."""
    S = np.stack([np.ones_like(idw), np.ones_like(idw), idw], axis=-1)        # [N][3]
    w = (p[None] - Q) * S[:, None, None, :]
    wc = w.mean(axis=2)                                                       # [N][M][3]
    rw = np.sqrt(((w - wc[:, :, None, :]) ** 2).sum(axis=-1).max(axis=-1))    # [N][M]
    need = 2.0 * np.maximum(1.0, idw)[:, None] * B[None, :] + r[:, None] + 2e-4 + rw
    return ~((wc * wc).sum(axis=-1) >= need * need)


def sphere_test(q, seg_bound, reach, radius, downwash):
    """(base [N][M], dist [N][M]) of agent q against every agent o, in float64 on the dumped float32 spheres and reach:
    base = s (2 B_m + 3 (rho_a + rho_o)) + r_a + r_o, dist = |S (C_a - C_o)|, S = diag(1, 1, 1 / downwash of the pair)."""
    sb = np.asarray(seg_bound, np.float64)
    B = np.asarray(reach, np.float64)[q]
    r = np.asarray(radius, np.float64)
    idw, s = pair_scale(r[q], float(downwash[q]), r, downwash)
    base = s[:, None] * (2.0 * B[None, :] + 3.0 * (sb[q, :, 3][None, :] + sb[:, :, 3])) + (r[q] + r)[:, None]
    d = sb[q, :, :3][None] - sb[:, :, :3]
    d[:, :, 2] *= idw[:, None]
    return base, np.sqrt((d * d).sum(axis=-1))


def priority_dist(state, q):
    """rule_distf (octomath::Vector3::distance) of every agent's position to agent q's: float32 differences, products and sums
    left to right, the square root in double.  float64 [N]."""
    pos = np.asarray(state, np.float32)[:, :3]
    d = (pos - pos[q]).astype(F)
    n2 = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F)
    n2 = (n2 + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
    return np.sqrt(n2.astype(np.float64))


def unit_index(q, N, M):
    """unit number o_i * M + m of every (agent o, segment m) as agent q's list counts them (o_i skips q itself); -1 in q's own row."""
    oi = np.arange(N) - (np.arange(N) > q)
    u = oi[:, None] * M + np.arange(M)[None, :]
    u[q] = -1
    return u


# ---- the closed form of the build kernel (reach_hi / reach_lo) in float32, for the CPU comparison with the sums
def reach_closed_form_f32(d0, V, A):
    """e_K for K = 1..27 [..., 27] as lsc_neigh_build_kernel forms it: float32 throughout, nh / nl by a floor of (V -+ d0) / A."""
    d0, V, A = (np.asarray(x, F) for x in (d0, V, A))
    with np.errstate(divide="ignore", invalid="ignore"):
        ia = np.where(A > 0, F(1.0) / A, F(0.0)).astype(F)
    nh = np.where(A > 0, np.maximum(np.floor(((V - d0).astype(F) * ia).astype(F)), F(0.0)), np.where(d0 <= V, F(1e9), F(0.0))).astype(F)
    nl = np.where(A > 0, np.maximum(np.floor(((d0 + V).astype(F) * ia).astype(F)), F(0.0)), np.where(d0 >= -V, F(1e9), F(0.0))).astype(F)
    out = []
    for K in range(1, 28):
        Kf = F(K)
        n1 = np.minimum(nh, Kf).astype(F)
        hi = (((n1 * d0).astype(F) + (((F(0.5) * A).astype(F) * n1).astype(F) * (n1 + F(1.0)).astype(F)).astype(F)).astype(F) + ((Kf - n1).astype(F) * V).astype(F)).astype(F)
        n1 = np.minimum(nl, Kf).astype(F)
        lo = (((n1 * d0).astype(F) - (((F(0.5) * A).astype(F) * n1).astype(F) * (n1 + F(1.0)).astype(F)).astype(F)).astype(F) - ((Kf - n1).astype(F) * V).astype(F)).astype(F)
        out.append(np.maximum(np.abs(lo), np.abs(hi)))
    return np.stack(out, axis=-1)
