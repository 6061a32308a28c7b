// lsc_flight.hip -- the flight record: MultiSyncSimulator's per-tick accounting on the device, one launch behind every tick of
// lsc_fly_device, one log row per tick (layout and every statement: lsc_flight.hpp).
//
//   isFinished                     (src/multi_sync_simulator.cpp:358-380)  -> summary.unmet     (on the tick's INPUT positions)
//   checkDeadlock's bookkeeping    (src/traj_planner.cpp:396-409)          -> summary.moved, summary.end_unmet
//   savePlanningResult             (src/multi_sync_simulator.cpp:446-503)  -> ratio, partner, summary.min_ratio
//   savePlanningResultAsCSV        (src/multi_sync_simulator.cpp:513-587)  -> samples, cost, status
//
// Shape.  A workgroup accounts for agents_per_block consecutive agents and never waits for another workgroup: it forms its share of
// the summary words in LDS and adds each word that is not zero with ONE atomic (integer adds, and a 64-bit unsigned minimum on the bits
// of a non-negative double: both independent of the order, so the row is the same bits in every run); the summaries were initialised
// by lsc_flight_begin / lsc_flight_reset.  Everything else leaves with plain vector stores.  The pair pass needs every partner's sample
// position: each workgroup evaluates them itself from traj_next (18 double multiply-adds per partner and time, the table is
// L2-resident) instead of reading what a sample kernel in front would have left -- a second dependent launch costs more than the
// redundant arithmetic up to about a thousand agents.
#include "lsc_kernels.h"
#include "lsc_flight.hpp"
#include "lsc_wave.hpp"

namespace lsc {

constexpr int FT = 256;                        // lanes of a record workgroup
constexpr int FLIGHT_WORDS = 9;                // summary words a workgroup adds to: unmet, end_unmet, moved, n_status[6]
constexpr int FLIGHT_MIN_OFFSET = 40;          // byte offset of lsc_flight_tick::min_ratio

__global__ __launch_bounds__(FT) void lsc_flight_kernel(const FlightArgs a)
{
#pragma clang fp contract(off)
    __shared__ int s_cnt[FLIGHT_WORDS];
    __shared__ double s_r[FT / 64];
    __shared__ int s_q[FT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, T = a.n_times;
    const int q0 = blockIdx.x * a.agents_per_block;
    const int nA = min(a.agents_per_block, N - q0);
    const FlightLayout L = flight_layout(N, T, a.what);
    if (tid < FLIGHT_WORDS) s_cnt[tid] = 0;
    __syncthreads();

    // ---- per agent: goal tests, end point, status; one lane per agent
    for (int al = tid; al < nA; al += FT) {
        const int q = q0 + al;
        const float *tn = a.traj_next + (size_t)q * NV;
        float e[3], ep[3];
        flight_end_point(tn, e);
        flight_end_point(a.traj_prev + (size_t)q * NV, ep);
        const int st = a.status[q];
        if (rule_goal_unmet(a.state + 9 * (size_t)q, a.goal + 3 * (size_t)q, a.goal_threshold)) atomicAdd(&s_cnt[0], 1);
        if (rule_goal_unmet(e, a.goal + 3 * (size_t)q, a.goal_threshold)) atomicAdd(&s_cnt[1], 1);
        if (flight_moved(e, ep, a.planner_seq)) atomicAdd(&s_cnt[2], 1);
        if (st >= 0 && st < 6) atomicAdd(&s_cnt[3 + st], 1);
        if (a.what & FLIGHT_AGENTS) {
            reinterpret_cast<double *>(a.row + L.cost)[q] = a.cost[q];
            reinterpret_cast<int *>(a.row + L.status)[q] = st;
            float *eo = reinterpret_cast<float *>(a.row + L.end) + 3 * (size_t)q;
            eo[0] = e[0]; eo[1] = e[1]; eo[2] = e[2];
        }
    }

    // ---- record samples: one lane per (agent, time, axis)
    if (a.what & FLIGHT_SAMPLES) {
        float *samples = reinterpret_cast<float *>(a.row + L.samples);
        for (int u = tid; u < nA * T * 3; u += FT) {
            const int al = u / (T * 3), r = u - al * (T * 3), ti = r / 3, k = r - ti * 3, q = q0 + al;
            const float *c = a.traj_next + (size_t)q * NV + k * SEGV + a.seg[ti] * NC;
            const FlightAxisSample s = flight_axis_sample(c, a.w5 + ti * 6, a.w4 + ti * 5, a.w3 + ti * 4, a.dt_inv);
            float *o = samples + ((size_t)ti * N + q) * 9;
            o[k] = s.p; o[3 + k] = s.v; o[6 + k] = s.a;
        }
    }

    // ---- agent-agent safety: the whole workgroup walks the partners of one agent and time, strided over the lanes in increasing index
    double block_min = FLIGHT_NO_PARTNER;
    if (a.what & FLIGHT_SAFETY) {
        double *ratio_out = reinterpret_cast<double *>(a.row + L.ratio);
        int *partner_out = reinterpret_cast<int *>(a.row + L.partner);
        for (int al = 0; al < nA; al++) {
            const int qi = q0 + al;
            const double r_a = a.radius[qi], dw_a = a.downwash[qi];
            for (int ti = 0; ti < T; ti++) {
                const int seg = a.seg[ti];
                const double *w = a.w5 + ti * 6;
                float pa[3];
                flight_position(a.traj_next + (size_t)qi * NV, seg, w, pa);
                double best = FLIGHT_NO_PARTNER;
                int bq = 0x7fffffff;
                for (int qj = tid; qj < N; qj += FT) {
                    if (qj == qi) continue;
                    float pb[3];
                    flight_position(a.traj_next + (size_t)qj * NV, seg, w, pb);
                    const double ratio = flight_pair_ratio(pa, pb, r_a, dw_a, a.radius[qj], a.downwash[qj]);
                    if (ratio < best) { best = ratio; bq = qj; }            // (increasing qj per lane: the first partner of a tie stays)
                }
                // smallest ratio, then smallest partner index
                const double wb = wave_min(best);
                int cand = best == wb ? bq : 0x7fffffff;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
                if (lane == 0) { s_r[wave] = wb; s_q[wave] = cand; }
                __syncthreads();
                if (tid == 0) {
                    double r = s_r[0];
                    int q = s_q[0];
                    for (int w2 = 1; w2 < FT / 64; w2++)
                        if (s_r[w2] < r || (s_r[w2] == r && s_q[w2] < q)) { r = s_r[w2]; q = s_q[w2]; }
                    ratio_out[(size_t)ti * N + qi] = r;
                    partner_out[(size_t)ti * N + qi] = q == 0x7fffffff ? -1 : q;
                    block_min = r < block_min ? r : block_min;
                }
                __syncthreads();
            }
        }
    }

    // ---- the workgroup's share of the summary: one atomic per word that has something to add
    __syncthreads();
    int *summary = reinterpret_cast<int *>(a.row);
    if (tid < FLIGHT_WORDS && s_cnt[tid] != 0) atomicAdd(summary + 1 + tid, s_cnt[tid]);
    if (tid == 0) {
        if (block_min < FLIGHT_NO_PARTNER)
            atomicMin(reinterpret_cast<unsigned long long *>(a.row + FLIGHT_MIN_OFFSET), (unsigned long long)__double_as_longlong(block_min));
        if (blockIdx.x == 0) summary[0] = a.planner_seq;
    }
}

__global__ void lsc_flight_init_kernel(unsigned char *rows, size_t row_bytes, int n_rows)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    int *s = reinterpret_cast<int *>(rows + (size_t)r * row_bytes);
    for (int i = 0; i < FLIGHT_SUMMARY_BYTES / 4; i++) s[i] = 0;
    *reinterpret_cast<double *>(rows + (size_t)r * row_bytes + FLIGHT_MIN_OFFSET) = FLIGHT_NO_PARTNER;
}

// Agents per workgroup.  With the pair pass a workgroup is busy with one agent for N / 256 rounds per time, so agents get a workgroup each
// until the grid would exceed about a thousand workgroups (four per CU); without it an agent is a lane's work.
int flight_agents_per_block(int N, int what)
{
    if (!(what & FLIGHT_SAFETY)) return 64;
    return N <= 1024 ? 1 : (N + 1023) / 1024;
}

hipError_t launch_flight(const FlightArgs &a, hipStream_t st, LaunchEvents ev)
{
    if (a.N < 1 || a.agents_per_block < 1 || a.n_times < 1 || a.n_times > FLIGHT_MAX_TIMES) return hipErrorInvalidValue;
    const int grid = (a.N + a.agents_per_block - 1) / a.agents_per_block;
    return launch_variant(kernel_address(lsc_flight_kernel), dim3(grid), dim3(FT), 0, st, a, ev);
}

hipError_t launch_flight_init(unsigned char *rows, size_t row_bytes, int n_rows, hipStream_t st)
{
    if (n_rows < 1) return hipSuccess;
    hipLaunchKernelGGL(lsc_flight_init_kernel, dim3((n_rows + 63) / 64), dim3(64), 0, st, rows, row_bytes, n_rows);
    return hipGetLastError();
}

}  // namespace lsc
