// lsc_obstacles.hip -- the mission's dynamic obstacles moved and recorded on the device (statements and layouts: lsc_obstacle_motion.hpp).
//
//   lsc_obstacle_kernel          the obstacle stage, the first launch of a tick of a context with motion models: getObstacle(t) of
//                                include/obstacle.hpp for every obstacle -> the [K][6] buffer ObsBlock::pos_vel points to
//   lsc_obstacle_step_kernel     the stage of a context with a chasing or gaussian model, launched INSTEAD of lsc_obstacle_kernel: the
//                                two kinds with state or history of their own beside the three closed forms, read - barrier - write
//   lsc_obstacle_record_kernel   the obstacle track, one launch behind lsc_flight_kernel in a recorded flight: savePlanningResult's
//                                obstacle ratio (src/multi_sync_simulator.cpp:480-500) and the tick's states -> one track row
//
// Shape.  The stage is one lane per obstacle in ONE workgroup of 64 (K <= 64), no LDS, no atomics: an obstacle's state is written by its
// lane alone, with plain vector stores, and read by the launches BEHIND it, which the stream orders.  The record is one lane per (record
// time, agent) pair, 256 lanes per workgroup over T N pairs; a lane forms its agent's sample position itself from traj_next (18 double
// multiply-adds) and walks the K obstacles in increasing index.  A workgroup never waits for another: it reduces its share of the two
// summary words in LDS and adds each with ONE atomic (an integer add, and a 64-bit unsigned minimum on the bits of a non-negative
// double: both independent of the order, so a row is the same bits in every run).  One more workgroup copies the states and the
// stage's positions in doubles.
#include "lsc_kernels.h"
#include "lsc_flight.hpp"
#include "lsc_obstacle_motion.hpp"
#include "lsc_wave.hpp"

namespace lsc {

constexpr int OT = 64;                         // lanes of the stage's one workgroup
constexpr int RT = 256;                        // lanes of a record workgroup

__global__ __launch_bounds__(OT) void lsc_obstacle_kernel(const ObstacleStageArgs a)
{
#pragma clang fp contract(off)
    const int o = threadIdx.x;
    if (o >= a.K) return;
    double p[3], v[3];
    obstacle_at(a.table[o], a.t, p, v);
    float *out = a.pos_vel + 6 * (size_t)o;
    out[0] = (float)p[0]; out[1] = (float)p[1]; out[2] = (float)p[2];
    out[3] = (float)v[0]; out[4] = (float)v[1]; out[5] = (float)v[2];
    double *exact = a.pos_f64 + 3 * (size_t)o;                         // (the same doubles, before the rounding)
    exact[0] = p[0]; exact[1] = p[1]; exact[2] = p[2];
}

// The stage of a context with at least one chasing or gaussian model, launched INSTEAD of lsc_obstacle_kernel: all five kinds, one
// lane per obstacle.  A chaser reads where the PREVIOUS tick put every other obstacle (updateObstacles: setObstacles for all, then
// getObstacle for all), so the order is read - barrier - write: every lane, those behind the K-th included, copies its own row of the
// previous tick's positions and its radius into LDS and reads its chaser state and its target's position of THIS tick's state buffer;
// all 64 lanes reach the one barrier; only then is anything stored, and behind the barrier nobody reads a row of global memory that
// another lane writes.  Before the first stage of an installation the previous obstacles are the generator's default-constructed ones
// (obstacle_generator.hpp:30, :108): positions 0 and radii 0.
__global__ __launch_bounds__(OT) void lsc_obstacle_step_kernel(const ObstacleStepArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_pos[OT][3];
    __shared__ double s_rad[OT];
    const int o = threadIdx.x;
    const bool live = o < a.K, prev = live && !a.first;
    const int kind = live ? a.table[o].kind : -1;
    for (int k = 0; k < 3; k++) s_pos[o][k] = prev ? a.pos_f64[3 * (size_t)o + k] : 0.0;
    s_rad[o] = prev ? a.obs->radius[o] : 0.0;                          // (ObsBlock::radius: (double)(float) r_o, the message's float32)
    ObstacleChaserState s = {};
    double goal[3] = {0.0, 0.0, 0.0};
    if (kind == OBSTACLE_CHASING) {
        const double *in = a.chaser_state + 7 * (size_t)o;
        for (int k = 0; k < 3; k++) { s.pos[k] = in[k]; s.vel[k] = in[3 + k]; }
        s.t_last = in[6];
        const float *target = a.state + 9 * (size_t)a.chasers[o].target;
        for (int k = 0; k < 3; k++) goal[k] = (double)target[k];
    }
    __syncthreads();
    if (!live) return;
    double p[3], v[3];
    if (kind == OBSTACLE_CHASING) {
        obstacle_chase_step(a.chasers[o], s, a.t, goal, s_pos, s_rad, a.K, o);
        double *out = a.chaser_state + 7 * (size_t)o;
        for (int k = 0; k < 3; k++) { out[k] = p[k] = s.pos[k]; out[3 + k] = v[k] = s.vel[k]; }
        out[6] = s.t_last;
    } else if (kind == OBSTACLE_GAUSSIAN) {
        const ObstacleWalker &w = a.walkers[o];
        obstacle_gaussian_at(w, reinterpret_cast<const double (*)[3]>(a.acc + 3 * (size_t)w.acc_first), a.t, p, v);
    } else {
        obstacle_at(a.table[o], a.t, p, v);
    }
    float *out = a.pos_vel + 6 * (size_t)o;
    out[0] = (float)p[0]; out[1] = (float)p[1]; out[2] = (float)p[2];
    out[3] = (float)v[0]; out[4] = (float)v[1]; out[5] = (float)v[2];
    double *exact = a.pos_f64 + 3 * (size_t)o;
    exact[0] = p[0]; exact[1] = p[1]; exact[2] = p[2];
}

__global__ __launch_bounds__(RT) void lsc_obstacle_record_kernel(const ObstacleRecordArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_min[RT / 64];
    __shared__ int s_below[RT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, T = a.n_times, K = a.K, pairs = N * T;
    const ObstacleTrackLayout L = obstacle_track_layout(N, T, K);
    if ((int)blockIdx.x == (pairs + RT - 1) / RT) {                     // the workgroup behind the pairs': the tick's states
        float *states = reinterpret_cast<float *>(a.row + L.states);
        for (int i = tid; i < 6 * K; i += RT) states[i] = a.pos_vel[i];
        double *positions = reinterpret_cast<double *>(a.row + L.positions);
        for (int i = tid; i < 3 * K; i += RT) positions[i] = a.pos_f64[i];
        return;
    }
    const int u = blockIdx.x * RT + tid;                               // = ti * N + q: the index of the row's [T][N] parts
    double best = OBSTACLE_NO_RATIO;
    if (u < pairs) {
        const int ti = u / N, q = u - ti * N;
        float pa[3];
        flight_position(a.traj_next + (size_t)q * NV, a.seg[ti], a.w5 + ti * 6, pa);
        const double r_a = a.radius[q];
        int bo = -1;
        for (int o = 0; o < K; o++) {
            const double ratio = rule_distf(pa, a.pos_vel + 6 * (size_t)o) / (r_a + a.obs->radius[o]);      // (ObsBlock::radius: (double)(float) r_o)
            if (ratio < best) { best = ratio; bo = o; }                // (strict, increasing o: the first obstacle of a tie stays)
        }
        reinterpret_cast<double *>(a.row + L.ratio)[u] = best;
        reinterpret_cast<int *>(a.row + L.partner)[u] = bo;
    }
    // ---- the workgroup's share of the summary: one atomic per word that has something to add
    const int below = __popcll(__ballot(best < 1.0));
    const double wmin = wave_min(best);
    if (lane == 0) { s_min[wave] = wmin; s_below[wave] = below; }
    __syncthreads();
    if (tid == 0) {
        double m = s_min[0];
        int b = s_below[0];
        for (int w = 1; w < RT / 64; w++) { m = s_min[w] < m ? s_min[w] : m; b += s_below[w]; }
        if (m < OBSTACLE_NO_RATIO) atomicMin(reinterpret_cast<unsigned long long *>(a.row), (unsigned long long)__double_as_longlong(m));
        if (b != 0) atomicAdd(reinterpret_cast<int *>(a.row + 8), b);
    }
}

__global__ void lsc_obstacle_track_init_kernel(unsigned char *rows, size_t row_bytes, int n_rows)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    unsigned char *row = rows + (size_t)r * row_bytes;
    *reinterpret_cast<double *>(row) = OBSTACLE_NO_RATIO;
    reinterpret_cast<int *>(row)[2] = 0;
    reinterpret_cast<int *>(row)[3] = 0;
}

hipError_t launch_obstacle_stage(const ObstacleStageArgs &a, hipStream_t st)
{
    if (a.K < 1 || a.K > OT || !a.table || !a.pos_vel || !a.pos_f64) return hipErrorInvalidValue;
    return launch_variant(kernel_address(lsc_obstacle_kernel), dim3(1), dim3(OT), 0, st, a);
}

hipError_t launch_obstacle_step(const ObstacleStepArgs &a, hipStream_t st)
{
    if (a.K < 1 || a.K > OT || !a.table || !a.chasers || !a.walkers || !a.obs || !a.state || !a.chaser_state || !a.pos_vel || !a.pos_f64) return hipErrorInvalidValue;
    return launch_variant(kernel_address(lsc_obstacle_step_kernel), dim3(1), dim3(OT), 0, st, a);
}

hipError_t launch_obstacle_record(const ObstacleRecordArgs &a, hipStream_t st)
{
    if (a.N < 1 || a.n_times < 1 || a.n_times > FLIGHT_MAX_TIMES || a.K < 1 || a.K > OBSTACLES_MAX || !a.row || !a.pos_vel || !a.pos_f64 || !a.obs || !a.traj_next)
        return hipErrorInvalidValue;
    const int grid = (a.N * a.n_times + RT - 1) / RT + 1;
    return launch_variant(kernel_address(lsc_obstacle_record_kernel), dim3(grid), dim3(RT), 0, st, a);
}

hipError_t launch_obstacle_track_init(unsigned char *rows, size_t row_bytes, int n_rows, hipStream_t st)
{
    if (n_rows < 1) return hipSuccess;
    hipLaunchKernelGGL(lsc_obstacle_track_init_kernel, dim3((n_rows + 63) / 64), dim3(64), 0, st, rows, row_bytes, n_rows);
    return hipGetLastError();
}

}  // namespace lsc
