"""The "pursuit" scenario of the chasing / gaussian obstacle tests (a plain module, imported like obstacle_reference): the 8-agent hover
mission with K = 5 obstacles that between them take every branch of getChasingObstacle and getGaussianObstacle
(tests/test_obstacle_reactive.py counts them):

    0, 1   two chasers with the same start, parameters and target: they stay coincident, so from the second step on each skips the other
           at dist < 1e-5
    2      a chaser aimed at another agent that starts 0.1 m from the origin: with the clock's now - start = 0.2 at the first tick its
           first step is taken against the generator's zero obstacles (radius 0: Q* = 2 r = 0.3 m > 0.1 m, the repulsion term) with dt > 0
    3      a walker with a 12-entry acceleration table at cycle 0.5
    4      a straight

gamma_target 5 against max_acc 1 clamps the acceleration at the first step (|a| = 5 x some metres), and max_vel 0.3 clamps the velocity
at the second (0.99 m/s^2 x 0.2 s per step).

The 12-entry table at cycle 0.5 serves times up to 6 s - 1e-5: ticks 1 .. 29 at dt 0.2 with the first tick at 0.2 s.  Flights of 30 and
40 ticks need 13 and 17 entries; pursuit(n_acc=17) is the same scenario with the table drawn on (its first 12 rows are the 12-entry
table's), so that no tick of those flights is dropped.
"""
import numpy as np

from obstacle_reference import hover_mission  # noqa: F401  (the scenario's mission)
from test_obstacle_motion import STRAIGHT

DT = 0.2
CLOCK = (0.0, 0.2, 0.2)          # lsc_obstacle_clock(start, now, step): the first tick evaluates at now - start = 0.2
WALKER_STDDEV, WALKER_MAX_ACC = 0.5, 1.0


def acc_table(n):
    """update_acc_history's draws and clip (include/obstacle.hpp:366-386) from a fixed seed; a longer table starts with the shorter one."""
    acc = np.random.default_rng(12).normal(0.0, WALKER_STDDEV, (64, 3))[:n]
    for a in acc:
        norm = float(np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]))
        if norm > WALKER_MAX_ACC:
            a[:] = a / norm * WALKER_MAX_ACC
    return acc


def chaser(start, target, size=0.2, **kw):
    o = {"type": "chasing", "start": list(map(float, start)), "size": size, "max_vel": 0.3, "max_acc": 1.0, "gamma_target": 5.0, "gamma_obs": 0.05,
         "downwash": 1.0, "target": target}
    o.update(kw)
    return o


def pursuit(n_acc=12):
    twin = chaser([0.5, 0.3, 1.6], 0)
    walker = {"type": "gaussian", "start": [-1.5, 1.0, 1.8], "initial_vel": [0.1, 0.0, 0.0], "size": 0.2, "max_vel": 0.25, "stddev_acc": WALKER_STDDEV,
              "max_acc": WALKER_MAX_ACC, "acc_update_cycle": 0.5, "downwash": 1.5, "acc_history": acc_table(n_acc).tolist()}
    return [twin, dict(twin), chaser([0.06, 0.08, 0.0], 3, size=0.15), walker, dict(STRAIGHT)]


def full_wave(n_agents=4, seed=64):
    """K = 64 chasers in a ball of 0.3 m, radius 0.5 each: every pair is inside its Q* = 2 m.  Six metres above the swarm: the plans are
    not the point."""
    rng = np.random.default_rng(seed)
    return [chaser(list(rng.uniform(-0.17, 0.17, 3) + [0.0, 0.0, 7.0]), k % n_agents, size=0.5, gamma_obs=0.2 + 0.01 * k, max_vel=0.2 + 0.002 * k)
            for k in range(64)]
