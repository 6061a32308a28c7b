"""The one table of parity tolerances.  Integer / byte / index work -- LSC normals and margins, corridor
boxes, distance fields, grid paths, planned goals, propagated states, statuses -- is compared bit for bit and has no entry
here.  The QP solve is floating point: north_star allows 1e-3 relative cost; the tests hold the kernel to

    cost          |gpu - oracle| <= COST_RTOL |oracle| + COST_ATOL
    control point |gpu - oracle| <= TRAJ_ATOL   (metres; float32 storage + flat directions of the cost; measured <= 1.5e-5)

Exceptions, each used by name where it applies:
"""
import os

from safety_certificate import storage_bound

COST_RTOL = 1e-6
COST_ATOL = 1e-8
TRAJ_ATOL = 2e-5
# LSC_SOLVER=interior_point (tests/test_gpu_round5.py runs the parity files once more through the interior point alone): that solver stops
# at a duality gap of 1e-9 (1 + |f|), which along flat directions of the cost leaves a plan up to ~1e-4 m from the optimum the oracle now
# returns exactly (measured 8.9e-5 m at tick 28 of the 20-agent circle, HiGHS arbitrating); rounds 1-4 compared two interior points, whose
# errors were similar.  The cost tolerance does not move.
#   The same bound holds wherever a test sends agents to the interior point on purpose -- solver = interior_point or hand_over, the second pass
#   with its rows in HBM (tests/test_gpu_highs_variants.py) --, so it has a name.
INTERIOR_POINT_TRAJ_ATOL = 1e-4
# (a test that names its solver itself is not moved by LSC_SOLVER: the active-set solve's bound under a name the switch below leaves alone)
ACTIVE_SET_TRAJ_ATOL = TRAJ_ATOL
if os.environ.get("LSC_SOLVER") == "interior_point":
    TRAJ_ATOL = INTERIOR_POINT_TRAJ_ATOL

# Seeded fuzzing of tiny swarms with extreme parameters (vmax 0.2..3, amax 0.5..6, radii 0.05..0.4, goals outside the world,
# coincident agents): optima with nearly flat directions -- the plan may move 3-4e-5 m at 1e-9 relative cost.
FUZZ_TRAJ_ATOL = 5e-5
# The same with dt = 0.5 (the M = 4 build): 2e-4 in round 4, for ONE genuinely flat optimum on which the oracle's and the kernel's interior
# points stopped on opposite sides of HiGHS's plan (tests/golden/fuzz_found_planar_m4_7500378.npz).  Since round 5 the oracle finishes its
# optimum exactly (oracle/lsc_oracle.c: orc_gi_polish) and the product's default solver is exact too: the exception is gone.
#   What is left at dt = 0.5 is the interior point's own tolerance: with half-second segments working sets beyond the active-set solve's
#   capacity (12 rows) are common, those agents are handed to the interior point, and an interior point that stops at a gap of 1e-9 (1 + |f|)
#   is up to ~1e-4 m off along flat directions of the cost (the TRAJ_ATOL of the interior-point-only runs above).  Found by the fuzzers in
#   round 5's last round: tests/golden/fuzz_found_m4_handover_8500018.npz -- a handed-over agent 5.8e-5 m from the oracle's plan at 4.2e-10
#   relative HIGHER cost, bit-identical to solver = interior_point (tests/test_gpu_round5.py).  Cost tolerance unchanged.
FUZZ_TRAJ_ATOL_HALF_SECOND = 1e-4
# ... and with the 1e5 slack penalty a grossly violated limit makes |f| ~ 1e7; both solvers stop on criteria relative to |f|
# and their plans may then differ by centimetres at 4e-8 relative cost: plans are compared below this objective only.
# (1e4 until round 4.  Slack-mode QPs can have a face of optima -- tests/golden/fuzz_found_7301082.npz: one value, no one plan -- and they
#  are the ones with a violated limit at penalty 1e5, i.e. with a large objective.  The cost comparison pins the optimum above the limit.)
FUZZ_PLAN_COMPARED_BELOW_COST = 1e3
# 1024-agent swarms near their goals: costs approach 0 (1e-6..1e-5), so the absolute floor is what binds.
LARGE_SWARM_COST_ATOL = 1e-7
# The same at the end of a mission flown to completion (tick 193 of the 64-agent bench mission: cost 2.4e-5, kernel and oracle
# 1.08e-8 apart): both solvers stop on criteria relative to 1 + |f|, i.e. absolute ones once f -> 0.
NEAR_GOAL_COST_ATOL = 1e-7

# Continuous-time separation of two agents that both solved their QP (tests/safety_certificate.py): the certified distance
# of a pair's segment may fall short of r_i + r_j by
#   (a) what float32 storage of an exact plan takes: safety_certificate.storage_bound of the mission's world box and smallest downwash
#       (6.8e-7 m in a +-5 m world, 3.6e-7 m in a +-3.2 m one), plus
#   (b) what the reference algorithm itself falls short by: its normals are float32 vectors of length 1 +- 6e-8, so the sum of the two
#       agents' rows certifies (r_i + r_j) / |n|.  Measured on the oracle's plans of every mission the certificate tests fly
#       (tests/test_safety_certificate.py re-flies them and holds each to this figure): at most 2.98e-9 m, on circle_swap(16, 3.0).
#       (The oracle's plans are stored as float32 too, so in a wide world its figure holds a share of (a): 4.8e-8 m on the 64-agent circle
#       of tests/test_gpu_properties.py, where (a) is 1.35e-6 m.  The kernels are held to 3e-9 there as well.)
# Neither part comes from the kernels.
ORACLE_SEPARATION_SHORTFALL = 3e-9


def separation_shortfall_bound(world_min, world_max, downwash):
    """dist - (r_i + r_j) >= -separation_shortfall_bound(...) is the assertion of every certificate test on the GPU."""
    return storage_bound(world_min, world_max, downwash) + ORACLE_SEPARATION_SHORTFALL
