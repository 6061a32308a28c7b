"""What the GPU tests share (a plain module, imported like tolerances and pin_variants): the closed loop on host buffers, the lockstep pair
of a default context and one held to a replaced path by an environment variable, and the comparison of a GPU tick with an oracle tick.

The loop asserts nothing: every comparison is an each_tick hook.  The two equality predicates are not the same -- same_bits tells -0.0
from +0.0 and takes equal NaN bits for equal, exact (np.array_equal) does neither -- and a test says which one it means.
"""
import numpy as np

from tolerances import COST_RTOL, TRAJ_ATOL


def start_inputs(ms, segv):
    """(state float32 [N][9] at rest at ms.start, zero trajectory table float32 [N][3][segv]); segv is the planner's SEGV."""
    n = len(ms.start)
    state = np.zeros((n, 9), np.float32); state[:, :3] = ms.start
    return state, np.zeros((n, 3, segv), np.float32)


def fly(planners, ms, ticks, *, goal=None, gusts=None, planar_z=None, each_tick=None, state=None, traj=None, **plan_kw):
    """Host-buffer ticks 1 .. ticks of one planner, or of several in lockstep on the same inputs; the first planner's plans feed the next
    tick.  gusts = {tick: (agent, offset)} moves an agent off its plan before that tick; planar_z clamps the propagated states to the plane.
    each_tick(tick, state, traj_in, outs) sees every tick's inputs and the planners' results; a true return value ends the flight.
    Returns the last tick flown."""
    from lsc_planner_amd.planner import next_state_host
    pls = list(planners) if isinstance(planners, (list, tuple)) else [planners]
    state0, traj0 = start_inputs(ms, pls[0].SEGV)
    state, traj = state0 if state is None else state, traj0 if traj is None else traj
    goal = ms.goal if goal is None else goal
    for tick in range(1, ticks + 1):
        if gusts and tick in gusts:
            q, off = gusts[tick]
            state[q, :3] += np.asarray(off, np.float32)
        outs = [pl.plan(state, goal, traj, **plan_kw) for pl in pls]
        if each_tick and each_tick(tick, state, traj, outs):
            return tick
        traj = outs[0]["traj"]
        state = next_state_host(traj, dt=pls[0].cfg.dt)
        if planar_z is not None:
            state[:, 2] = planar_z; state[:, 5] = 0.0; state[:, 8] = 0.0
    return ticks


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def exact(a, b):
    return np.array_equal(a, b)


def assert_lockstep(new, old, tick, outs, *, eq=same_bits, keys=("traj", "cost", "status", "iters"), diagnostics=("last_goals", "row_counts")):
    """One tick of two planners on the same inputs: the named results, and what the named planner methods return, are equal."""
    gn, go = outs
    for k in keys:
        assert eq(gn[k], go[k]), (tick, k)
    for name in diagnostics:
        x, y = getattr(new, name)(), getattr(old, name)()
        assert (x == y) if isinstance(x, dict) else eq(x, y), (tick, name, x, y)


def held_planner(L, ms, cfg, monkeypatch, env, hold, note=None):
    """A context created with env set (hold) or absent; env is absent again afterwards.  note, if given, must be in the context's note."""
    if hold:
        monkeypatch.setenv(env, "1")
    else:
        monkeypatch.delenv(env, raising=False)
    pl = L.SwarmPlanner(ms, cfg() if callable(cfg) else cfg)
    monkeypatch.delenv(env, raising=False)
    assert note is None or note in pl.note(), pl.note()
    return pl


def held_pair(L, ms, cfg, monkeypatch, env, new_note=None, old_note=None):
    """(default context, context held to the replaced path by env at its creation), each checked through its note."""
    return held_planner(L, ms, cfg, monkeypatch, env, False, new_note), held_planner(L, ms, cfg, monkeypatch, env, True, old_note)


def assert_tick_matches(g, o, where, *, rows=True, cost_atol=0.0, traj_atol=TRAJ_ATOL, traj_mask=None):
    """GPU tick g against oracle (or reference) tick o on the same inputs.  rows: normals and margins equal -- True or "exact" by value,
    "bits" through their integer views, False not at all --; statuses equal; cost of the oracle's status-0 agents within
    COST_RTOL |cost| + cost_atol; plans (of the agents in traj_mask, if given) within traj_atol."""
    if rows:
        for k, u in (("normal", np.uint32), ("d", np.uint64)):
            a, b = (g[k].view(u), o[k].view(u)) if rows == "bits" else (g[k], o[k])
            assert np.array_equal(a, b), (where, k)
    assert np.array_equal(g["status"], o["status"]), (where, g["status"], o["status"])
    ok = o["status"] == 0
    assert (np.abs(g["cost"] - o["cost"])[ok] <= COST_RTOL * np.abs(o["cost"])[ok] + cost_atol).all(), (where, g["cost"], o["cost"])
    err = np.abs(g["traj"] - o["traj"])
    err = (err if traj_mask is None else err[traj_mask]).max(initial=0.0)
    assert err <= traj_atol, (where, err)


def assert_same_flights(a, b, names, what=""):
    """Two flights, each a list of ticks of lists of missions of the named fields (numpy arrays or torch tensors): every field equal."""
    import torch
    assert len(a) == len(b), (what, len(a), len(b))
    for tick, (ta, tb) in enumerate(zip(a, b), 1):
        assert len(ta) == len(tb), (what, tick)
        for m, (ma, mb) in enumerate(zip(ta, tb)):
            assert len(ma) == len(mb), (what, tick, m)
            for k, (x, y) in enumerate(zip(ma, mb)):
                same = torch.equal(x, y) if torch.is_tensor(x) else np.array_equal(x, y)
                assert same, (what, "tick", tick, "mission", m, names[k])


def circle(L, n, radius):
    return L.circle_swap(n, circle_radius=radius, z=1.0, world=(-radius - 2, -radius - 2, 0, radius + 2, radius + 2, 2.5))
