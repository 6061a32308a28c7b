"""The obstacle track of a recorded flight, restated in numpy: savePlanningResult's obstacle ratio (src/multi_sync_simulator.cpp:480-500).

A plain float32 distance with no downwash -- differences, products and their sum in float32, left to right, the square root in double
(octomath::Vector3::distance: rule_distf of csrc/lsc_rules.hpp) -- over r_a + (double)(float) r_o, a double division; the obstacle stays
where the TICK put it at every record time; the partner is the FIRST obstacle attaining the minimum.
"""
import numpy as np


def track_reference(samples, pos_vel, agent_radius, obstacle_radius):
    """samples float32 [n][T][N][9] (the flight log's), pos_vel float32 [n][K][6] (the tick's states), radii float64 [N], [K]
    -> (ratio float64 [n][T][N], partner int32 [n][T][N])."""
    p = np.asarray(samples, np.float32)[..., :3]
    o = np.asarray(pos_vel, np.float32)[:, :, :3]
    d = p[:, :, :, None, :] - o[:, None, None, :, :]                       # float32 [n][T][N][K][3]
    n2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    assert d.dtype == np.float32 and n2.dtype == np.float32
    r_a = np.asarray(agent_radius, np.float64)[None, None, :, None]
    r_o = np.asarray(obstacle_radius, np.float64).astype(np.float32).astype(np.float64)[None, None, None, :]
    ratio = np.sqrt(n2.astype(np.float64)) / (r_a + r_o)
    return ratio.min(axis=-1), ratio.argmin(axis=-1).astype(np.int32)      # (argmin: the first of a tie)
