"""-m gpu: goal planning of small swarms on a wave of its own beside the GJK pass (csrc/lsc_kernels.hip, the wave roles of plan_agent)
against the generic path (LSC_GENERIC_LSC_BUILD at context creation), which plans the goal in front of the GJK pass, by all waves.

Every test flies a default context and a generic-pass context in lockstep on the same inputs and compares the same arrays bit for bit,
like tests/test_gpu_small_swarm_build.py.  What that file's missions do not force is forced here: a retreat whose partner is found by
the goal wave's argmin with two partners at the same distance, a partner and a disturbed agent that only the scan's SECOND round
(agent 64 of a 65-agent swarm) sees, and the first tick with static goals on the kernel without the alternate-mode hooks.
"""
import numpy as np
import pytest

from harness import assert_lockstep, circle, fly, held_pair, same_bits, start_inputs

pytestmark = pytest.mark.gpu

ENV = "LSC_GENERIC_LSC_BUILD"
NEW, OLD = "lsc build: one wave per segment", "lsc build: generic pass (LSC_GENERIC_LSC_BUILD)"


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle
    return oracle


def _mission(L, start, goal, half=14.0):
    n = len(start)
    ms = L.circle_swap(n, circle_radius=1.0, z=1.0, world=(-half, -half, 0, half, half, 2.5))
    ms.start = np.asarray(start, np.float32)
    ms.goal = np.asarray(goal, np.float32)
    return ms


def _fly(new, old, ms, ticks, gusts=None, each_tick=None):
    """Both contexts in lockstep on host buffers; each_tick(tick, state, traj, gn) sees every tick's inputs and the default context's
    outputs."""
    def same(tick, state, traj, outs):
        assert_lockstep(new, old, tick, outs, diagnostics=("last_goals", "row_counts", "bucket_max"))
        if each_tick:
            each_tick(tick, state, traj, outs[0])
    fly((new, old), ms, ticks, gusts=gusts, each_tick=same)


def _retreat_mission(L, d, swapped):
    """Agent 1 at the origin with a far goal; agents 0 and 2 at -d and +d (swapped: +d and -d), each 1 m from its own goal: both have
    priority over agent 1, both are inside priority_dist_threshold, at the SAME float32 distance."""
    s = -1.0 if not swapped else 1.0
    start = [(s * d, 0, 1), (0, 0, 1), (-s * d, 0, 1)]
    goal = [(s * d, 1, 1), (5, 0, 1), (-s * d, 1, 1)]
    return _mission(L, start, goal, half=7.0)


@pytest.mark.parametrize("d", [0.3, 0.35])
def test_retreat_with_a_tie(L, oracle, monkeypatch, d):
    """The retreat branch with two partners at equal distance: the lower index wins, its position is read from the lane that holds it.
    0.3 m is the contact distance of the default radii, 0.35 m lies inside priority_dist_threshold (0.4)."""
    got = []
    for swapped in (False, True):
        ms = _retreat_mission(L, d, swapped)
        new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15), monkeypatch, ENV, NEW, OLD)
        state, traj0 = start_inputs(ms, new.SEGV)
        ref = oracle.goal_prior_based(state, ms.goal, traj0, 1)
        clamped = oracle.goal_prior_based(state, ms.goal, traj0, 1, priority_dist_threshold=0.0)      # (nobody is that close: no retreat)
        assert np.allclose(clamped[1], [2, 0, 1])
        # the oracle itself, checked here: away from agent 0, the lower index of the two partners, to priority_dist_threshold + 0.1
        assert np.allclose(ref[1], [-0.5 if swapped else 0.5, 0, 1], atol=1e-6), ref[1]
        assert same_bits(ref[[0, 2]], clamped[[0, 2]])                # (the outer agents have priority: they keep their goals)

        def first_tick(tick, state, traj, gn, new=new, ref=ref, clamped=clamped):
            if tick == 1:
                assert same_bits(new.last_goals(), ref), (new.last_goals(), ref)
                assert not np.array_equal(new.last_goals()[1], clamped[1])          # the retreat branch was taken
                got.append(float(new.last_goals()[1][0]))
        _fly(new, old, ms, 3, each_tick=first_tick)
        new.close(); old.close()
    assert got[0] > 0.0 and got[1] < 0.0 and got[0] == -got[1], got      # the swapped order flips the sign


def _second_round_mission(L, mirrored):
    """65 agents: agent 0 at the origin with a far goal, its only partner inside 0.4 m is agent 64 -- the scan's second round -- at 0.35 m, 1 m
    from its goal; agents 1 .. 63 on a circle of 12 m.  mirrored: agent 3 sits at -0.35 m as well, the lower index of a tie across the rounds."""
    ms = L.circle_swap(63, circle_radius=12.0, z=1.0, world=(-14, -14, 0, 14, 14, 2.5))
    start = np.concatenate([[(0, 0, 1)], ms.start, [(0.35, 0, 1)]]).astype(np.float32)
    goal = np.concatenate([[(8, 0, 1)], ms.goal, [(0.35, 1, 1)]]).astype(np.float32)
    if mirrored:
        start[3] = (-0.35, 0, 1); goal[3] = (-0.35, 1, 1)
    return _mission(L, start, goal)


@pytest.mark.parametrize("mirrored", [False, True])
def test_second_scan_round(L, oracle, monkeypatch, mirrored):
    """N = 65 (64 obstacles: still one wave per segment): the partner of the retreat is agent 64, which lane 0 of the goal wave meets in its
    second round; with agent 3 mirrored the two are tied and the lower index, of the first round, must win."""
    ms = _second_round_mission(L, mirrored)
    assert ms.qn == 65
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15), monkeypatch, ENV, NEW, OLD)

    def goals_of_the_oracle(tick, state, traj, gn):
        ref = oracle.goal_prior_based(state, ms.goal, traj, tick)
        if tick == 1:
            assert np.allclose(ref[0], [0.5 if mirrored else -0.5, 0, 1], atol=1e-6), ref[0]      # (the oracle itself: away from 3 / from 64)
        assert same_bits(new.last_goals(), ref), (tick, np.nonzero((new.last_goals() != ref).any(1))[0])
    _fly(new, old, ms, 3, each_tick=goals_of_the_oracle)
    new.close(); old.close()


def test_disturbance_seen_by_the_second_round(L, monkeypatch):
    """A gust on agent 64 alone (0.25 m, beyond reset_threshold 0.15) at tick 4: the flag comes from the second round of the goal wave's scan,
    and from that tick on every agent of both contexts is planned by the folded general solver -- none by the plan kernel's own solve."""
    ms = circle(L, 65, 8.0 * 65 / 64.0)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15), monkeypatch, ENV, NEW, OLD)
    ran_here = {}

    def count(tick, state, traj, gn):
        st = new.solver_stats()
        ran_here[tick] = st["solved"] + st["handed_over"]
        so = old.solver_stats()
        assert ran_here[tick] == so["solved"] + so["handed_over"], tick
    _fly(new, old, ms, 8, gusts={4: (64, (0.25, 0.0, 0.0))}, each_tick=count)
    assert ran_here[3] > ran_here[2] > ran_here[1] > 0, ran_here
    assert all(ran_here[t] == ran_here[3] for t in range(4, 9)), ran_here
    new.close(); old.close()


def test_first_tick_static_goals(L, monkeypatch):
    """Two agents, static goals, reset_threshold 0 (lsc_plan_kernel, without the alternate-mode hooks): tick 1 builds the initial trajectories
    from the states (planner_seq < 2), and the goal wave writes the goal input through."""
    ms = _mission(L, [(-1.0, 0.1, 1), (1.0, -0.1, 1)], [(1.0, 0, 1), (-1.0, 0, 1)], half=5.0)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="static", reset_threshold=0.0), monkeypatch, ENV, NEW, OLD)

    def goals_are_the_input(tick, state, traj, gn):
        assert same_bits(new.last_goals(), ms.goal), tick
    _fly(new, old, ms, 3, each_tick=goals_are_the_input)
    new.close(); old.close()
