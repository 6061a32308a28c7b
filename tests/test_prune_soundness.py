"""What phase B's row pruning rests on, proven on the CPU by LP (HiGHS, the copy SciPy bundles, with the tolerances of tests/highs_qp.py)
on the oracle's own rows (oracle.qp_assemble(...).dense(); tests/test_oracle_qp.py pins those to the reference's QPmodel.lp).  Comparing
optima cannot see a wrong box -- the wrongly dropped rows are simply not active at the optimum --, so:

    a  the box of tests/prune_reference.py holds every point the reference's velocity, acceleration and continuity rows allow;
    b  every row the rule drops is redundant in the agent's polytope, on the scenes the GPU tests use;
    c  on those scenes the COUNT of kept rows moves under every wrong rule tried, which is what tests/test_gpu_prune_rule.py holds
       the kernels by;
    d  rows so close to the threshold that another order of additions may decide them otherwise are at most 1 % of the candidates.
"""
import functools

import numpy as np
import pytest

import highs_qp as H
import prune_scenes as PS
from neighbour_reference import state_constants
from prune_reference import BAND, limits, reach_bounds, steps_of

pytestmark = pytest.mark.skipif(not H.available(), reason="SciPy's HiGHS is not importable")

LP_TOL = 1e-9            # HiGHS's primal feasibility tolerance as highs_qp._new sets it: an LP optimum may sit that far outside a row
FAMILIES = {"3d_m5": (False, 5, 0.2), "planar_m5": (True, 5, 0.2), "3d_m4": (False, 4, 0.5), "planar_m4": (True, 4, 0.5)}
Z2D = 0.9
lps_solved = [0]


class Polytope:
    """The rows of an oracle.QP as one HiGHS model whose cost is changed between runs (the basis of the last run starts the next)."""

    def __init__(self, qp, with_bounds=True):
        Aeq, beq, G, h = qp.dense()
        if not with_bounds:
            nb = int(np.isfinite(qp.lo).sum() + np.isfinite(qp.hi).sum())          # dense() appends the variable bounds behind the rows
            G, h = G[:len(G) - nb], h[:len(h) - nb]
        self.n = qp.nv
        A = np.vstack([Aeq, G])
        lo, hi = np.r_[beq, np.full(len(h), -np.inf)], np.r_[beq, h]
        self.h = H._new()
        free = np.full(self.n, np.inf)
        H._pass_lp(self.h, np.zeros(self.n), A, lo, hi, -free, free)
        self.h.run()
        lps_solved[0] += 1
        self.empty = self.h.modelStatusToString(self.h.getModelStatus()) != "Optimal"
        self.cols = np.arange(self.n, dtype=np.int32)

    def minimum(self, cost):
        self.h.changeColsCost(self.n, self.cols, np.asarray(cost, np.float64))
        self.h.run()
        lps_solved[0] += 1
        st = self.h.modelStatusToString(self.h.getModelStatus())
        assert st == "Optimal", st
        return float(self.h.getInfo().objective_function_value)


def _zero_obstacle_qp(O, prm, state, goal, vnom, vmax, amax):
    e = np.zeros((0, 3, O.SEGV), np.float32)
    return O.qp_assemble(prm, state, goal, vnom, vmax, amax, e, np.zeros((0, O.M, 3), np.float32), np.zeros((0, O.M, 6)))


# ------------------------------------------------------------------------------------------------- a
def _draw_states(rng, n, planar, dt):
    """States rounded to float32 as the kernel reads them: at rest; |v| at 0.5, 0.97 and exactly 1.0 of vmax per axis with mixed signs;
    a = 0 and |a| up to amax; vmax in 0.3 .. 2.5, amax in 0.5 .. 6 (d0 - j A reaches the -V clamp within 27 steps for some, not for
    others).  An acceleration that pushes the first step beyond V empties the polytope; three in four of those are turned inwards."""
    out = []
    for t in range(n):
        vmax = np.repeat(np.float32(rng.uniform(0.3, 2.5)), 3).astype(np.float64)       # float32 values: v = vmax exactly is representable
        amax = np.repeat(rng.uniform(0.5, 6.0), 3)
        s = np.zeros(9, np.float32)
        s[:3] = rng.uniform(-1.0, 1.0, 3)
        if t > 0:
            frac = rng.choice([0.0, 0.5, 0.97, 1.0], 3) if t % 4 else np.full(3, rng.choice([0.5, 0.97, 1.0]))
            s[3:6] = rng.choice([-1.0, 1.0], 3) * frac * vmax
            acc = np.where(rng.random(3) < 0.4, 0.0, rng.uniform(-1.0, 1.0, 3)) * amax
            V, A = limits(vmax, amax, dt)
            d0 = s[3:6].astype(np.float64) * (dt / 5) + acc * (dt * dt / 20)
            outward = np.abs(d0) > V
            if rng.random() < 0.75:
                acc = np.where(outward, -acc, acc)
            s[6:9] = acc
        if planar:
            s[2], s[5], s[8] = Z2D, 0.0, 0.0
        out.append((s, vmax, amax))
    return out


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_box_holds_every_point_of_the_reference_polytope(oracle, family):
    """2a.  The zero-obstacle QP of one agent (a world so large that its box never binds: the rule does not use it); for every control
    point with K >= 1 and every axis the LP minimum and maximum of c_{m,i} - c_{0,2}: lo[K] <= min and max <= hi[K], the LP's own error
    allowed as K 1e-9 -- HiGHS's primal feasibility tolerance once per step.  Measured: smallest slack 1.0e-9 in every family, the pad
    itself at K = 1; largest 1.01 m (3-D, M = 5), 0.99 m (planar), 1.82 m and 2.12 m (M = 4); 3 + 8 + 1 + 2 of 4 x 30 states empty.  Both
    are printed."""
    O = oracle
    planar, M, dt = FAMILIES[family]
    rng = np.random.default_rng(41 + list(FAMILIES).index(family))
    kw = dict(world_dimension=2, world_z_2d=Z2D) if planar else {}
    checked = empty = 0
    smallest, largest = np.inf, -np.inf
    with O.segments(M):
        prm = O.make_params(dt=dt, world_min=(-100, -100, -100), world_max=(100, 100, 100), obs_f32=True, **kw)
        K = steps_of(M).reshape(-1)
        for s, vmax, amax in _draw_states(rng, 30, planar, dt):
            qp = _zero_obstacle_qp(O, prm, s, s[:3] + np.float32(1.0), 1.0, vmax, amax)
            poly = Polytope(qp)
            if poly.empty:
                empty += 1
                continue
            checked += 1
            c02, d0 = state_constants(s[None], dt, planar, Z2D)
            V, A = limits(vmax, amax, dt)
            lo, hi = reach_bounds(d0[0], V, A)                                           # [3][28]
            for k in range(2 if planar else 3):
                for cp in range(3, O.SEGV):
                    cost = np.zeros(qp.nv)
                    cost[k * O.SEGV + cp], cost[k * O.SEGV + 2] = 1.0, -1.0
                    mn, mx = poly.minimum(cost), -poly.minimum(-cost)
                    tol = K[cp] * LP_TOL
                    assert lo[k, K[cp]] <= mn + tol and mx - tol <= hi[k, K[cp]], (family, s, vmax, amax, k, cp, lo[k, K[cp]], mn, mx, hi[k, K[cp]])
                    smallest, largest = min(smallest, mn - lo[k, K[cp]], hi[k, K[cp]] - mx), max(largest, mn - lo[k, K[cp]], hi[k, K[cp]] - mx)
    print(f"2a {family}: {checked} states checked, {empty} skipped as empty; smallest slack {smallest:.3e}, largest {largest:.3e}; LPs so far {lps_solved[0]}")
    assert checked >= 20, (checked, empty)


# ------------------------------------------------------------------------------------------------- the scene sets
@functools.lru_cache(maxsize=None)
def _sweep_rows(oracle_mod, every=1, companions=0, planar=False, m4=False, tick=False):
    """[(name, D, state, goal, pred, normal, d, prm, mission)] of a sweep family at tick 1.  tick: the rows are those of the oracle's own
    tick (Swarm.tick(want_lsc=True), which also solves the QPs) and tests/prune_scenes.PairRows, which composes them from
    oracle.lsc_pair without a solve, is held to them; otherwise PairRows alone."""
    O = oracle_mod
    M, dt = (4, 0.5) if m4 else (5, 0.2)
    n = 2 + companions
    out = []
    with O.segments(M):
        ms = PS.mission(n, companions=companions, planar_z=Z2D if planar else None)
        kw = dict(world_dimension=2, world_z_2d=Z2D) if planar else {}
        prm = O.make_params(dt=dt, world_min=ms.world_min, world_max=ms.world_max, obs_f32=True, **kw)
        sw = O.Swarm(prm, ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
        prev = np.zeros((n, 3, O.SEGV), np.float32)
        pairs = PS.PairRows(O, ms.radius, ms.downwash)
        for name, D, state, goal in PS.sweep_scenes(n, PS.PLANAR_SWEEPS if planar else PS.SWEEPS, every, companions, Z2D if planar else None):
            pred = PS.predictions(O, state, prev, 1, dt)
            normal, d = pairs.rows(pred)
            if tick:
                sw.stale[:] = 0
                o = sw.tick(state, goal, prev, 1, want_lsc=True)
                assert np.array_equal(normal, o["normal"]) and np.array_equal(d, o["d"]), (name, D)
            out.append((name, D, state, goal, pred, normal.copy(), d.copy(), prm, ms))
    return out


@functools.lru_cache(maxsize=None)
def _threshold_scenes(oracle_mod):
    O = oracle_mod
    out = []
    for name, u, frac in PS.SWEEPS:
        for D in PS.THRESHOLD_DISTANCES:
            t = PS.threshold_scene(O, u, frac, D)
            if t is not None:
                out.append((name, D) + t)
    return out


def _fuzz_ticks(O, seeds, ticks=4):
    """The oracle's own closed loop on the swarms of the fuzz generator: yields (seed, tick, f, prm, state, goal, prev, pred, o)."""
    for seed in seeds:
        f = PS.fuzz_swarm(seed)
        n = len(f["start"])
        prm = O.make_params(world_min=f["wmin"], world_max=f["wmax"], obs_f32=True)
        sw = O.Swarm(prm, f["radius"], f["dw"], f["vmax"], f["amax"], f["vnom"])
        state = np.zeros((n, 9), np.float32)
        state[:, :3], state[:, 3:6] = f["start"], f["vel0"]
        prev = np.zeros((n, 3, O.SEGV), np.float32)
        for tick in range(1, ticks + 1):
            o = sw.tick(state, f["goal"], prev, tick, want_lsc=True)
            yield seed, tick, f, prm, state, f["goal"], prev, PS.predictions(O, state, prev, tick, 0.2), o
            prev = o["traj"]
            state = np.array([O.next_state(prev[q]) for q in range(n)], np.float32)


# ------------------------------------------------------------------------------------------------- b
def _certify(O, prm, state, goal, vnom, vmax, amax, pts, normal, d, keep, planar=False):
    """LP minimum of n . c_{m,i} - rhs over the agent's velocity, acceleration and continuity rows (no world box: the rule does not use
    it) for every dropped row; returns (rows certified, smallest minimum) or None when the polytope is empty."""
    qp = _zero_obstacle_qp(O, prm, state, goal, vnom, vmax, amax)
    poly = Polytope(qp, with_bounds=False)
    if poly.empty:
        return None
    n = np.array(normal, np.float64)
    if planar:
        n[..., 2] = 0.0
    rhs = d + (n[:, :, None, :] * pts).sum(axis=-1)
    K = steps_of(n.shape[1])
    count, worst = 0, np.inf
    for o, m, i in np.argwhere(~keep & (K >= 1)[None]):
        cost = np.zeros(qp.nv)
        for k in range(2 if planar else 3):
            cost[k * O.SEGV + m * 6 + i] = n[o, m, k]
        mn = poly.minimum(cost) - rhs[o, m, i]
        assert mn >= 0.0, ("a dropped row is not redundant", o, m, i, mn, state, n[o, m], rhs[o, m, i])
        count, worst = count + 1, min(worst, mn)
    return count, worst


def test_every_dropped_row_is_redundant(oracle):
    """2b.  The sweep at every fourth distance (and every sixteenth of the planar and the four-segment sweeps) and the fuzz generator's swarms of 2 .. 8 agents at
    ticks 1 .. 4: for every row kept_rows drops, the LP minimum of n . c_{m,i} - rhs over the agent's polytope is >= 0."""
    O = oracle
    agents = checked = rows = 0
    smallest = np.inf

    def one(prm, state, goal, pred, normal, d, vnom, vmax, amax, dt, planar):
        nonlocal agents, checked, rows, smallest
        kept = PS.kept_of_tick(state, pred, normal, d, vmax, amax, dt, planar=planar, z2d=Z2D)
        pts = PS.points_of(pred)
        for q, (keep, gap, _) in kept.items():
            agents += 1
            r = _certify(O, prm, state[q], goal[q], vnom[q], vmax[q], amax[q], np.delete(pts, q, axis=0), normal[q], d[q], keep, planar)
            if r is not None:
                checked += 1
                rows += r[0]
                smallest = min(smallest, r[1])

    for planar, m4, every in ((False, False, 4), (True, False, 16), (False, True, 16)):
        M, dt = (4, 0.5) if m4 else (5, 0.2)
        with O.segments(M):
            for name, D, state, goal, pred, normal, d, prm, ms in _sweep_rows(O, every, 0, planar, m4, True):
                one(prm, state, goal, pred, normal, d, ms.nominal_velocity, ms.max_vel, ms.max_acc, dt, planar)
    n_sweep = rows
    for seed, tick, f, prm, state, goal, prev, pred, o in _fuzz_ticks(O, range(300, 306)):
        one(prm, state, goal, pred, o["normal"], o["d"], f["vnom"], f["vmax"], f["amax"], 0.2, False)
    print(f"2b: {agents} agents, {checked} with a non-empty polytope, {rows} dropped rows certified ({n_sweep} on the sweeps); "
          f"smallest LP minimum of a dropped row {smallest:.3e}; LPs so far {lps_solved[0]}")
    assert 2 * checked >= agents and rows >= 1000, (agents, checked, rows)


# ------------------------------------------------------------------------------------------------- c, d
MUTATIONS = {"K + 1": dict(shift=1), "K - 1": dict(shift=-1), "reachL / reachU swapped": dict(swap=True), "pad's sign flipped": dict(pad=-1)}


def _scene_counts(O, scenes, dt, planar, **rule):
    """[(count, fullest bucket) per agent] per scene"""
    out = []
    for name, D, state, goal, pred, normal, d, prm, ms in scenes:
        kept = PS.kept_of_tick(state, pred, normal, d, ms.max_vel, ms.max_acc, dt, planar=planar, z2d=Z2D, **rule)
        out.append(tuple((int(k.sum()), int(c.max())) for k, g, c in kept.values()))
    return out


def _threshold_as_sweep(O):
    out = []
    for name, D, radius, state, goal, row in _threshold_scenes(O):
        ms = PS.mission(2, radius=radius)
        pred = PS.predictions(O, state, None, 1, 0.2)
        normal, d = PS.PairRows(O, ms.radius, ms.downwash).rows(pred)
        out.append((name, D, state, goal, pred, normal, d, None, ms))
    return out


def test_the_count_moves_under_every_wrong_rule(oracle):
    """2c.  Per-agent kept count and fullest bucket on the sweep (with the threshold scenes, which are what resolves a pad of 1e-9)
    differ from those of the rule in at least 10 scenes for each of K + 1, K - 1, the bounds swapped and the pad's sign flipped."""
    O = oracle
    scenes = _sweep_rows(O) + _threshold_as_sweep(O)
    rule = _scene_counts(O, scenes, 0.2, False)
    ranges = {}
    for name, mut in MUTATIONS.items():
        wrong = _scene_counts(O, scenes, 0.2, False, mutate=mut)
        differ = sum(a != b for a, b in zip(rule, wrong))
        ranges[name] = (differ, min(c for s in wrong for c, _ in s), max(c for s in wrong for c, _ in s))
    print("2c: kept rows per agent under the rule", min(c for s in rule for c, _ in s), "..", max(c for s in rule for c, _ in s),
          "| scenes that differ, range of counts:", ranges)
    for name, (differ, _, _) in ranges.items():
        assert differ >= 10, (name, ranges)


def test_borderline_rows_are_rare(oracle):
    """2d.  |worst - (rhs + 1e-6)| <= 1e-9 for at most 1 % of the candidate rows of every scene set the GPU tests use (the closed loops
    there run on the kernel's own plans; tests/test_gpu_prune_rule.py asserts the same cap on the ticks it flies)."""
    O = oracle
    sets = {}

    def add(name, kept):
        e, c = sets.get(name, (0, 0))
        for keep, gap, _ in kept.values():
            e, c = e + int((np.abs(gap) <= BAND).sum()), c + int(np.isfinite(gap).sum())
        sets[name] = (e, c)

    for name, (comp, planar, m4) in {"sweep": (0, False, False), "companions": (2, False, False), "planar": (0, True, False), "m4": (0, False, True)}.items():
        M, dt = (4, 0.5) if m4 else (5, 0.2)
        with O.segments(M):
            for _, D, state, goal, pred, normal, d, prm, ms in _sweep_rows(O, 1, comp, planar, m4):
                add(name, PS.kept_of_tick(state, pred, normal, d, ms.max_vel, ms.max_acc, dt, planar=planar, z2d=Z2D))
    for _, D, state, goal, pred, normal, d, prm, ms in _threshold_as_sweep(O):
        add("threshold", PS.kept_of_tick(state, pred, normal, d, ms.max_vel, ms.max_acc, 0.2))
    for seed, tick, f, prm, state, goal, prev, pred, o in _fuzz_ticks(O, range(300, 340), ticks=6):
        add("closed loop", PS.kept_of_tick(state, pred, o["normal"], o["d"], f["vmax"], f["amax"], 0.2))
    print("2d: (borderline, candidate rows)", sets)
    for name, (e, c) in sets.items():
        assert c > 0 and e <= 0.01 * c, (name, e, c)


# ------------------------------------------------------------------------------------------------- the table of DESIGN section 4.1
def optimum_table(O, every=1):
    """What comparing optima sees of a wrong rule (python tests/test_prune_soundness.py): every scene of the seven sweeps solved with all
    27 rows and with the rows a rule drops relaxed (margin -1e6); per rule the number of sweeps in which no plan moved by one bit and the
    largest plan difference in the others."""
    rules = {"the rule": {}, "K - 1": dict(shift=-1), "K - 3": dict(shift=-3), "K - 5": dict(shift=-5), "swapped": dict(swap=True)}
    out = {k: {} for k in rules}
    for name, D, state, goal, pred, normal, d, prm, ms in _sweep_rows(O, every):
        for q in range(2):
            obs = np.delete(pred, q, axis=0)
            solve = lambda dd: O.qp_assemble(prm, state[q], goal[q], ms.nominal_velocity[q], ms.max_vel[q], ms.max_acc[q], obs, normal[q], dd).solve()
            st0, x0 = solve(d[q])[:2]
            for rule, mut in rules.items():
                keep = PS.kept_of_tick(state, pred, normal, d, ms.max_vel, ms.max_acc, 0.2, agents=[q], mutate=mut)[q][0]
                st, x = solve(np.where(keep | (steps_of(5) < 1)[None], d[q], -1e6))[:2]
                diff = np.inf if st != st0 else (float(np.abs(x.astype(np.float32) - x0.astype(np.float32)).max()) if st0 == 0 else 0.0)
                out[rule][name] = max(out[rule].get(name, 0.0), diff)
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as O_
    for rule, sweeps in optimum_table(O_).items():
        same = [n for n, v in sweeps.items() if v == 0.0]
        print(f"{rule:10s} unchanged in {len(same)} of {len(sweeps)} sweeps; others:", {n: f"{v:.2e}" for n, v in sweeps.items() if v != 0.0})
