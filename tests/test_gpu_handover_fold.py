"""-m gpu: the hand-over of disturbed agents solved inside the plan kernel (lsc_plan_alt_kernel + general_fold, csrc/lsc_general.hpp)
against the two-launch path it replaces (the plan kernel, then lsc_general_kernel; forced by LSC_GENERAL_HANDOVER at context creation).

Gusts push agents off their plans (farther than reset_threshold), so that phase A flags them and the swarm is handed over at some ticks
and not at others.  Both paths must give the same bits: plans, costs, statuses, iteration counts -- on host-buffer ticks and on
device-resident ticks (the benchmark's form) -- and the folded path must still match the oracle on the flagged ticks.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from harness import assert_lockstep, assert_tick_matches, exact, fly, held_pair, held_planner, start_inputs
from tolerances import COST_ATOL

ENV = "LSC_GENERAL_HANDOVER"

GUSTS = {5: (3, (0.25, -0.2, 0.0)), 9: (0, (-0.2, 0.15, 0.05)), 14: (6, (0.1, 0.3, 0.0))}


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


@pytest.mark.parametrize("goal_mode", ["static", "prior_based"])
def test_folded_hand_over_is_the_two_launch_path_bit_for_bit(L, monkeypatch, goal_mode):
    ms = L.circle_swap(12, 2.0, world=(-5, -5, 0, 5, 5, 2.5))
    cfg = L.PlannerConfig(goal_mode=goal_mode, reset_threshold=0.15)
    fold, two = held_pair(L, ms, cfg, monkeypatch, ENV)

    def same(tick, state, traj, outs):
        assert_lockstep(fold, two, tick, outs, eq=exact, diagnostics=())
        assert (outs[0]["status"] != 6).all(), tick                # (nobody left handed over and unsolved)
    fly((fold, two), ms, 18, gusts=GUSTS, each_tick=same)
    fold.close(); two.close()


def test_folded_hand_over_on_device_resident_ticks(L, monkeypatch):
    """The benchmark's form: prior_based goals, lsc_tick_device (the host never sees the states), gusts between ticks."""
    import torch
    from lsc_planner_amd.planner import next_state_host
    ms = L.circle_swap(16, 2.0, world=(-5, -5, 0, 5, 5, 2.5))
    N = ms.qn
    cfg = L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15)
    pls = held_pair(L, ms, cfg, monkeypatch, ENV)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    goal = torch.from_numpy(ms.goal).to(dev)
    state0 = start_inputs(ms, pls[0].SEGV)[0]
    runs = []
    for pl in pls:
        state = torch.from_numpy(state0).to(dev)
        traj = torch.zeros((N, 90), device=dev)
        out = []
        for tick in range(1, 21):
            if tick in GUSTS:
                q, off = GUSTS[tick]
                state[q, :3] += torch.tensor(off, dtype=torch.float32, device=dev)
            nxt = torch.zeros((N, 90), device=dev)
            cost = torch.zeros(N, dtype=torch.float64, device=dev)
            status = torch.zeros(N, dtype=torch.int32, device=dev)
            iters = torch.zeros(N, dtype=torch.int32, device=dev)
            pl.tick_device(state, goal, traj, nxt, cost, status, iters, tick, st)
            torch.cuda.synchronize()
            out.append((nxt.cpu().numpy(), cost.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()))
            traj = nxt
            state = torch.from_numpy(next_state_host(nxt.cpu().numpy().reshape(N, 3, 30))).to(dev)
        runs.append(out)
        pl.close()
    for tick, (f, t) in enumerate(zip(*runs), 1):
        for k, (a, b) in enumerate(zip(f, t)):
            assert np.array_equal(a, b), (tick, ("traj", "cost", "status", "iters")[k])
        assert (f[2] != 6).all(), (tick, f[2])


def test_folded_hand_over_matches_the_oracle(L, oracle, monkeypatch):
    """Every tick against the oracle; the gusts flag agents, so that from tick 5 on the whole swarm is solved by the folded general
    solver (its slack set only grows)."""
    from lsc_planner_amd.planner import next_state_host
    O = oracle
    ms = L.circle_swap(8, 1.5, world=(-5, -5, 0, 5, 5, 2.5))
    pl = held_planner(L, ms, L.PlannerConfig(reset_threshold=0.15), monkeypatch, ENV, False)
    prm = O.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True)
    sw = O.SwarmEx(prm, O.make_modes(reset_threshold=0.15), ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
    state, traj = start_inputs(ms, pl.SEGV)
    stale = np.zeros_like(traj)
    flagged = 0
    for tick in range(1, 17):
        if tick in GUSTS:
            q, off = GUSTS[tick]
            state[q, :3] += np.asarray(off, np.float32)
        own = sw.disturbance_update(state, traj, tick)
        flagged += int(np.asarray(own).sum())
        g = pl.plan(state, ms.goal, traj, want_constraints=True)
        sw.stale[:] = stale
        o = sw.tick(state, ms.goal, traj, tick, want_lsc=True, nthreads=8)
        assert_tick_matches(g, o, tick, cost_atol=COST_ATOL)
        ok = o["status"] == 0
        stale = np.where(ok[:, None, None], g["traj"], stale).astype(np.float32)
        traj = g["traj"]; state = next_state_host(traj)
    pl.close()
    assert flagged >= 2, flagged
    assert sw.slack_set.any()
