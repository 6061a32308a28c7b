"""tests/harness.py held to the CPU oracle: the oracle plays the planner (4 agents, three ticks, one thread), so the loop, the lockstep
comparison, the two predicates, the tick comparison and the held pair are exercised without a GPU."""
import copy
import os
import types

import numpy as np
import pytest

from conftest import oracle_swarm
from harness import assert_lockstep, assert_tick_matches, exact, fly, held_pair, same_bits, start_inputs
from tolerances import COST_RTOL, TRAJ_ATOL


class _OraclePlanner:
    """plan / SEGV / cfg.dt / last_goals / row_counts over the oracle's tick; spoil(out) may alter a tick's result before it is returned."""

    def __init__(self, O, ms, spoil=None):
        self.sw, self.SEGV, self.cfg, self.seq, self.spoil = oracle_swarm(O, ms), O.SEGV, types.SimpleNamespace(dt=0.2), 0, spoil
        self.inputs, self.rows = [], 0

    def plan(self, state, goal, traj, **kw):
        self.seq += 1
        self.inputs.append((state.copy(), traj.copy(), kw))
        self.sw.stale[:] = traj
        out = self.sw.tick(state, goal, traj, self.seq, want_lsc=True, nthreads=1)
        self.goals, self.rows = np.array(goal, np.float32), (out["d"] != 0).any(axis=(2, 3)).sum(1).astype(np.int32)
        if self.spoil:
            self.spoil(self, out)
        return out

    def last_goals(self):
        return self.goals

    def row_counts(self):
        return self.rows


@pytest.fixture(scope="module")
def ms():
    import lsc_planner_amd as L
    return L.circle_swap(4, 1.0)


def _hook(pls):
    return lambda tick, state, traj, outs: assert_lockstep(pls[0], pls[1], tick, outs)


def test_fly_feeds_both_planners_the_same_inputs(oracle, ms):
    from lsc_planner_amd.planner import next_state_host
    pls = [_OraclePlanner(oracle, ms), _OraclePlanner(oracle, ms)]
    seen = []

    def hook(tick, state, traj, outs):
        seen.append((tick, state.copy(), traj.copy(), outs))
        return _hook(pls)(tick, state, traj, outs)
    gust = (1, (0.05, -0.03, 0.0))
    assert fly(pls, ms, 3, gusts={2: gust}, planar_z=1.25, each_tick=hook, want_constraints=True) == 3
    assert [t for t, *_ in seen] == [1, 2, 3]
    s0, t0 = start_inputs(ms, pls[0].SEGV)
    assert s0.dtype == np.float32 and s0.shape == (4, 9) and exact(s0[:, :3], ms.start) and not s0[:, 3:].any()
    assert t0.dtype == np.float32 and t0.shape == (4, 3, pls[0].SEGV) and not t0.any()
    for k, (tick, state, traj, outs) in enumerate(seen):
        for pl in pls:                                   # both planners saw the hook's inputs, and the keywords of plan
            assert same_bits(pl.inputs[k][0], state) and same_bits(pl.inputs[k][1], traj) and pl.inputs[k][2] == {"want_constraints": True}
        if k == 0:
            assert same_bits(state, s0) and same_bits(traj, t0)
            continue
        want = next_state_host(seen[k - 1][3][0]["traj"], dt=0.2)          # the first planner's plan, propagated ...
        want[:, 2] = 1.25; want[:, 5] = 0.0; want[:, 8] = 0.0              # ... clamped to the plane ...
        if tick == 2:
            want[gust[0], :3] += np.asarray(gust[1], np.float32)           # ... and pushed by the gust before its tick
        assert same_bits(state, want), tick
        assert same_bits(traj, seen[k - 1][3][0]["traj"])


def test_fly_ends_on_a_true_return_and_takes_its_own_start(oracle, ms):
    pl = _OraclePlanner(oracle, ms)
    state, traj = start_inputs(ms, pl.SEGV)
    state[:, 3] = 0.1
    goal = ms.goal + np.float32(0.25)
    assert fly(pl, ms, 5, goal=goal, state=state, traj=traj, each_tick=lambda tick, *_: tick == 2) == 2
    assert pl.seq == 2 and same_bits(pl.inputs[0][0], state) and same_bits(pl.goals, goal)


def _flip_traj(pl, out):
    out["traj"].view(np.uint32)[2, 1, 7] ^= 1


def _change_status(pl, out):
    out["status"][3] += 1


def _change_diagnostic(pl, out):
    pl.rows = pl.rows.copy(); pl.rows[0] += 1


@pytest.mark.parametrize("spoil,word", [(_flip_traj, "traj"), (_change_status, "status"), (_change_diagnostic, "row_counts")])
def test_assert_lockstep_sees_a_difference(oracle, ms, spoil, word):
    """The second planner's tick 2 differs in one low bit of one control point, in one status, in one diagnostic: named with its tick."""
    pls = [_OraclePlanner(oracle, ms), _OraclePlanner(oracle, ms, spoil=lambda pl, out: pl.seq == 2 and spoil(pl, out))]
    ticks = []
    with pytest.raises(AssertionError, match=r"\(2, '%s'" % word):
        fly(pls, ms, 3, each_tick=lambda tick, *a: ticks.append(tick) or _hook(pls)(tick, *a))
    assert ticks == [1, 2]


def test_the_two_predicates_differ():
    plus, minus = np.array([0.0], np.float32), np.array([-0.0], np.float32)
    assert not same_bits(plus, minus) and exact(plus, minus)
    nan = np.array([np.nan, 1.0], np.float32)
    assert same_bits(nan, nan.copy()) and not exact(nan, nan.copy())
    assert not same_bits(np.zeros(2, np.float32), np.zeros(2, np.float64)) and not same_bits(np.zeros(2), np.zeros((2, 1)))


@pytest.fixture(scope="module")
def tick(oracle, ms):
    """One oracle tick (the second of the mission, so that the plans move) with its rows; left unchanged by the tests."""
    pl = _OraclePlanner(oracle, ms)
    outs = []
    fly(pl, ms, 2, each_tick=lambda t, s, tr, o: outs.append(o[0]))
    o = outs[-1]
    assert (o["status"] == 0).all() and (np.abs(o["cost"]) > 1e-3).all()
    return o


def _altered(o, key, index, value=None, flip=None):
    g = copy.deepcopy(o)
    if flip is not None:
        g[key].view(flip)[index] ^= 1
    else:
        g[key][index] = value
    return g


def test_assert_tick_matches(tick):
    o = tick
    assert_tick_matches(o, o, "same")
    assert_tick_matches(o, o, "same", rows="bits")
    for rows in ("exact", "bits"):
        with pytest.raises(AssertionError):
            assert_tick_matches(_altered(o, "normal", (1, 0, 2, 1), flip=np.uint32), o, rows, rows=rows)
        with pytest.raises(AssertionError):
            assert_tick_matches(_altered(o, "d", (1, 0, 2, 1), flip=np.uint64), o, rows, rows=rows)
    assert_tick_matches(_altered(o, "normal", (1, 0, 2, 1), flip=np.uint32), o, "rows not compared", rows=False)
    with pytest.raises(AssertionError):
        assert_tick_matches(_altered(o, "status", 2, 1), o, "status")
    off = 2 * COST_RTOL * abs(o["cost"][1])
    g = _altered(o, "cost", 1, o["cost"][1] + off)
    with pytest.raises(AssertionError):
        assert_tick_matches(g, o, "cost", cost_atol=0.0)
    assert_tick_matches(g, o, "cost under the floor", cost_atol=off)
    g = _altered(o, "traj", (3, 0, 4), o["traj"][3, 0, 4] + np.float32(2 * TRAJ_ATOL))
    with pytest.raises(AssertionError):
        assert_tick_matches(g, o, "plan")
    assert_tick_matches(g, o, "plan, wider bound", traj_atol=4 * TRAJ_ATOL)
    assert_tick_matches(g, o, "plan, agent 3 masked out", traj_mask=np.arange(4) != 3)
    with pytest.raises(AssertionError):
        assert_tick_matches(g, o, "plan, agent 3 alone", traj_mask=np.arange(4) == 3)


def test_assert_tick_matches_ignores_the_cost_of_failed_agents(tick):
    o = _altered(tick, "status", 2, 1)                  # the oracle's agent 2 failed: its cost says nothing
    g = _altered(o, "cost", 2, 1e9)
    assert_tick_matches(g, o, "failed agent")
    with pytest.raises(AssertionError):
        assert_tick_matches(_altered(o, "cost", 1, 1e9), o, "solved agent")


class _StubPlanner:
    def __init__(self, ms, cfg):
        self.cfg, self.env = cfg, os.environ.get("LSC_STUB")

    def note(self):
        return "held" if self.env else "default"


def test_held_pair_sets_the_variable_for_the_second_creation_only(ms, monkeypatch):
    L = types.SimpleNamespace(SwarmPlanner=_StubPlanner)
    monkeypatch.setenv("LSC_STUB", "left over")
    made = []
    new, old = held_pair(L, ms, lambda: made.append(1) or len(made), monkeypatch, "LSC_STUB", "default", "held")
    assert new.env is None and old.env == "1" and "LSC_STUB" not in os.environ
    assert (new.cfg, old.cfg) == (1, 2)                 # a callable config is called once per context
    new, old = held_pair(L, ms, "cfg", monkeypatch, "LSC_STUB", "default", "held")
    assert new.cfg == old.cfg == "cfg"
    with pytest.raises(AssertionError):
        held_pair(L, ms, "cfg", monkeypatch, "LSC_STUB", "default", "another path")
    with pytest.raises(AssertionError):
        held_pair(L, ms, "cfg", monkeypatch, "LSC_STUB", "another path", "held")
    assert "LSC_STUB" not in os.environ
