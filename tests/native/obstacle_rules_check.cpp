// Test-only: compiles the product's rules header (csrc/lsc_rules.hpp) for the HOST and prints the two rules of the dynamic obstacles --
// rule_obstacle_segment and rule_pair_downwash -- on the inputs it reads, as bit patterns, so that the CPU test-suite can hold them to
// the oracle's const_vel_traj and to the reference's two downwash formulas bit for bit without a GPU.  Not part of the product library.
//
// stdin, one case per line:  six hex words (float32 bits of pos | vel), the hex bits of the double dt, four hex words of doubles (r_a dw_a r_o dw_o)
// stdout, one line per case: M * 6 * 3 hex words (segment m, control point i, axis k), then the agent and the non-agent downwash (hex doubles)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "../../lsc_planner_amd/csrc/lsc_rules.hpp"

using namespace lsc;

int main()
{
    uint32_t w[6];
    uint64_t q[5];
    while (std::scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64,
                      &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &q[0], &q[1], &q[2], &q[3], &q[4]) == 11) {
        float pv[6];
        double d[5];
        std::memcpy(pv, w, sizeof pv);
        std::memcpy(d, q, sizeof d);
        for (int m = 0; m < M; m++) {
            F3 out[6];
            rule_obstacle_segment(pv, m, (float)d[0], out);
            for (int i = 0; i < 6; i++) {
                const float c[3] = {out[i].x, out[i].y, out[i].z};
                uint32_t b[3];
                std::memcpy(b, c, sizeof b);
                std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " ", b[0], b[1], b[2]);
            }
        }
        const double dw[2] = {rule_pair_downwash(d[1], d[2], d[3], d[4], true), rule_pair_downwash(d[1], d[2], d[3], d[4], false)};
        uint64_t b[2];
        std::memcpy(b, dw, sizeof b);
        std::printf("%016" PRIx64 " %016" PRIx64 "\n", b[0], b[1]);
    }
    return 0;
}
