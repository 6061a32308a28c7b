// Test-only: compiles the corridor kernel's per-axis cell rule (rule_sfc_axis_cells, csrc/lsc_rules.hpp) for the HOST, so that the CPU
// test-suite can walk it over every lattice index against the reference's literal samples (tests/test_sfc_axis_cells.py).  Not part of
// the product library.
#include <cmath>
#include "../../lsc_planner_amd/csrc/lsc_rules.hpp"

using namespace lsc;

// the bound lsc_set_distmap refuses worlds at
extern "C" double sfchdr_world_reach_max() { return SFC_WORLD_REACH_MAX; }

// n slabs [lo[j], hi[j]] of one axis -> out[j] = {a0, b0, b1}
extern "C" void sfchdr_axis_cells(int n, const double *lo, const double *hi, double wres, double rf, int kmin, const double *wmin, int *out)
{
    for (int j = 0; j < n; j++) {
        const SfcAxisCells c = rule_sfc_axis_cells(lo[j], hi[j], wres, rf, kmin, wmin[j]);
        out[3 * j] = c.a0; out[3 * j + 1] = c.b0; out[3 * j + 2] = c.b1;
    }
}
