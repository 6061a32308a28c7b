// lsc_kernels.hip -- gfx950 kernels of the replanning tick (one workgroup of 256 lanes per agent).
//
//   lsc_plan_kernel      : prediction shift -> LSC build (GJK, pruning, bucketing) -> reduced-space
//                          primal-dual interior point QP -> float32 trajectory      (the hot path)
//   lsc_sweep_kernel     : dense LSC sweep for every ordered (agent, obstacle, segment) -> HBM
//   lsc_propagate_kernel : next ideal state from the planned trajectory at t = dt
//   lsc_gjk_kernel       : batched GJK test hook
//
// Reference behaviour being replaced (file:line in /root/reference):
//   TrajPlanner::obstaclePredictionWithPrevSol / initialTrajPlanningPrevSol  src/traj_planner.cpp:829-864, 997-1016
//   TrajPlanner::generateLSC                                                 src/traj_planner.cpp:1310-1407
//   TrajOptimizer::populatebyrow + IloCplex::solve                           src/traj_optimizer.cpp:261-539, 76-96
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "lsc_general.hpp"
#include "lsc_gjk.hpp"
#include "lsc_model.hpp"
#include "lsc_kernels.h"
#include "lsc_rules.hpp"
#include "lsc_wave.hpp"

namespace lsc {

constexpr int NT = 512;      // lanes per agent workgroup: 8 waves, 2 per SIMD (register budget 256 per lane)
constexpr int NWAVE = NT / 64;

// ---------------------------------------------------------------------------------------------------
// Dense LSC sweep: one lane per (agent, obstacle, segment).  Output is what CollisionConstraints holds
// after generateLSC (normal shared by the 6 rows of a segment, six margins).
// ---------------------------------------------------------------------------------------------------
// F32: the six margins as float32 (12 + 24 B per segment: the 180 B per pair of SURVEY 8(d)); else as the doubles the QP reads
template <bool F32>
__global__ __launch_bounds__(256) void lsc_sweep_kernel(SweepArgs a)
{
    const int n_obs = a.N - 1;
    const long total = (long)a.count * n_obs * M;
    for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long)gridDim.x * blockDim.x) {
        const int m = (int)(u % M);
        const int oi = (int)((u / M) % n_obs);
        const int al = (int)(u / ((long)M * n_obs));
        const int qi = a.first + al;
        const int qj = oi < qi ? oi : oi + 1;
        F3 pa[6], po[6];
        load_segment(a.state, a.traj_prev, qi, m, a.planner_seq, a.dtf, pa);
        load_segment(a.state, a.traj_prev, qj, m, a.planner_seq, a.dtf, po);
        const double r_a = a.radius[qi], r_o = a.radius_obs[qj];
        const double downwash = (a.downwash[qi] * r_a + a.downwash_obs[qj] * r_o) / (r_a + r_o);
        F3 n;
        double d[6];
        lsc_segment(pa, po, downwash, r_o + r_a, n, d);
        float *on = a.out_normal + u * 3;
        on[0] = n.x; on[1] = n.y; on[2] = n.z;
        if constexpr (F32) {
            float *od = a.out_d32 + u * 6;
#pragma unroll
            for (int i = 0; i < 6; i++) od[i] = (float)d[i];
        } else {
            double *od = a.out_d + u * 6;
#pragma unroll
            for (int i = 0; i < 6; i++) od[i] = d[i];
        }
    }
}

__global__ __launch_bounds__(256) void lsc_gjk_kernel(const double *__restrict__ pts, int count, double *__restrict__ v,
                                                      double *__restrict__ dist)
{
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    const double *p = pts + (size_t)c * 18;
    D3 q[6];
#pragma unroll
    for (int i = 0; i < 6; i++) q[i] = D3{p[3 * i], p[3 * i + 1], p[3 * i + 2]};
    D3 w;
    int nv;
    dist[c] = gjk_origin_hull6(q[0], q[1], q[2], q[3], q[4], q[5], w, nv);
    v[3 * c] = w.x; v[3 * c + 1] = w.y; v[3 * c + 2] = w.z;
}

// getStateFromControlPoints at t = dt (include/polynomial.hpp:63-97): segment 1, local time 0.
__global__ void lsc_propagate_kernel(const float *__restrict__ traj, float *__restrict__ state, int N, float finv)
{
#pragma clang fp contract(off)   // the reference evaluates these float32 expressions without fusing
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * 3) return;
    int q = idx / 3, k = idx % 3;
    const float *c1 = traj + (size_t)q * NV + k * SEGV + NC;
    const float fn = (float)DEG, fn1 = (float)(DEG - 1);
    float v0 = ((c1[1] - c1[0]) * fn) * finv;
    float v1 = ((c1[2] - c1[1]) * fn) * finv;
    float a0 = ((v1 - v0) * fn1) * finv;
    state[9 * q + k] = c1[0];
    state[9 * q + 3 + k] = v0;
    state[9 * q + 6 + k] = a0;
}


// ---------------------------------------------------------------------------------------------------
// Safe Flight Corridor: CorridorConstructor::expandBoxFromPoint (include/corridor_constructor.hpp:18-245) driven by
// TrajPlanner::generateFeasibleSFC (src/traj_planner.cpp:1451-1491).  The reference tests every lattice point of a
// slab against the distance field; here "distance < margin" is pre-thresholded into a 3-D integral image, so a slab
// test is 64 independent loads.  One wave per agent, speculative over the growth steps (see sfc_expand).
// ---------------------------------------------------------------------------------------------------
struct SfcGrid {
    const int *I;
    int nx, ny, nz;
    int kmin[3];
    double rf, wres;
    double wmin[3], wmax[3];
};

// isObstacleInBox (:81-122).  Per axis the reference visits the lattice points lo, lo+res, ..., each nudged by a
// float 1e-5: the first one downwards (unless the box sits on the world boundary), all others upwards.  In cells that
// is {a0} u [b0, b1] per axis (rule_sfc_axis_cells, lsc_rules.hpp) -- note that the cell just above `lo` is skipped by the
// reference, so the tested set is the product of those per-axis sets: 8 sub-boxes, each answered by the integral image.
__device__ bool sfc_blocked(const SfcGrid &g, const double *box)
{
#pragma clang fp contract(off)
    int a0[3], b0[3], b1[3];
    const int dims[3] = {g.nx, g.ny, g.nz};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const SfcAxisCells c = rule_sfc_axis_cells(box[i], box[i + 3], g.wres, g.rf, g.kmin[i], g.wmin[i]);
        a0[i] = c.a0; b0[i] = c.b0; b1[i] = c.b1;
        if (a0[i] < 0 || a0[i] >= dims[i] || b0[i] < 0 || b1[i] >= dims[i]) return true;   // getDistance() = -1 outside
    }
    const int sy = g.nz + 1, sx = (g.ny + 1) * (g.nz + 1);
    int cnt = 0;
#pragma unroll
    for (int sel = 0; sel < 8; sel++) {
        const int x0 = (sel & 1) ? b0[0] : a0[0], x1 = ((sel & 1) ? b1[0] : a0[0]) + 1;
        const int y0 = (sel & 2) ? b0[1] : a0[1], y1 = ((sel & 2) ? b1[1] : a0[1]) + 1;
        const int z0 = (sel & 4) ? b0[2] : a0[2], z1 = ((sel & 4) ? b1[2] : a0[2]) + 1;
        const int *I = g.I;
        cnt += I[x1 * sx + y1 * sy + z1] - I[x0 * sx + y1 * sy + z1] - I[x1 * sx + y0 * sy + z1] - I[x1 * sx + y1 * sy + z0] +
               I[x0 * sx + y0 * sy + z1] + I[x0 * sx + y1 * sy + z0] + I[x1 * sx + y0 * sy + z0] - I[x0 * sx + y0 * sy + z0];
    }
    return cnt > 0;
}

__device__ bool sfc_in_boundary(const SfcGrid &g, const double *b)
{
    return b[0] > g.wmin[0] - 1e-9 && b[1] > g.wmin[1] - 1e-9 && b[2] > g.wmin[2] - 1e-9 && b[3] < g.wmax[0] + 1e-9 &&
           b[4] < g.wmax[1] + 1e-9 && b[5] < g.wmax[2] + 1e-9;
}

// returns 0 ok, 1 seed box blocked, 2 seed outside the world.  Executed by ONE WAVE per box (all 64 lanes call it
// with the same arguments and return the same result).
//
// The reference grows the box one resolution step at a time, round-robin over the directions that are still free
// (expand_box :184-232): inherently sequential, a few hundred dependent slab tests.  Here the wave speculates: lane
// l assumes that the l-1 steps before it all pass, rebuilds the box the reference would hold at that point and tests
// its own slab; the first failing lane (ballot) is exactly the reference's first failure, everything before it is
// accepted at once, that direction is dropped and the next round starts.  A box costs ~10 rounds of independent
// loads instead of hundreds of dependent ones.
//
// Box faces only ever take the values  seed -/+ res -/+ res ...  (repeated additions, which is what the reference
// does and what makes the doubles bit-identical), independently per face, so the six sequences are tabulated once in
// LDS (T[face][count]) and "the box after s steps" is six table reads at counts that follow from the round-robin.
__device__ int sfc_expand(const SfcGrid &g, const float point[3], const float goal[3], double out[6], double *T, int TL)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    double cur[6];
    for (int i = 0; i < 3; i++) {
        const double p = (double)point[i];
        const double rp = round(p / g.wres) * g.wres;
        if (fabs(p - rp) < 0.01) { cur[i] = rp; cur[i + 3] = rp; }
        else { cur[i] = floor(p / g.wres) * g.wres; cur[i + 3] = ceil(p / g.wres) * g.wres; }
    }
    if (sfc_blocked(g, cur)) return 1;
    // setAxisCand (:142-182): axes ordered by |goal - centre|, goal-ward direction first, opposite directions reversed
    unsigned cpack = 0;          // direction list, 3 bits each
    int ncand = 6;
    {
        int cand[6];
        float delta[3];
        double val[3];
        int offs[3], order[3], n = 0;
        for (int k = 0; k < 3; k++) {
            const float mid = (float)(0.5 * (cur[k] + cur[k + 3]));
            delta[k] = goal[k] - mid;
            offs[k] = delta[k] > 0 ? 3 : 0;
            val[k] = fabs((double)delta[k]);
        }
        double maxv = -1.0, minv = 1e9;
        for (int i = 0; i < 3; i++) {
            if (val[i] > maxv) { for (int j = n; j > 0; j--) order[j] = order[j - 1]; order[0] = i; n++; maxv = val[i]; }
            else if (val[i] < minv) { order[n++] = i; minv = val[i]; }
            else { for (int j = n; j > 1; j--) order[j] = order[j - 1]; order[1] = i; n++; }
        }
        for (int i = 0; i < 3; i++) { cand[i] = order[i] + offs[order[i]]; cand[5 - i] = order[i] + (3 - offs[order[i]]); }
        for (int j = 0; j < 6; j++) cpack |= (unsigned)cand[j] << (3 * j);
    }
    // face tables: lanes 0..5 run the six chains of additions
    if (lane < 6) {
        double v = lane == 0 ? cur[0] : lane == 1 ? cur[1] : lane == 2 ? cur[2] : lane == 3 ? cur[3] : lane == 4 ? cur[4] : cur[5];
        double *t = T + lane * TL;
        const double step = lane < 3 ? -g.wres : g.wres;
        // (one dependent addition per entry, in the reference's order; unrolled, the loop's own instructions no longer stand between them)
#pragma unroll 8
        for (int k = 0; k < TL; k++) { t[k] = v; v = v + step; }
    }
    __syncthreads();
    int cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0, cnt4 = 0, cnt5 = 0;   // accepted expansions per face (wave-uniform)
    int i = -1;
    bool fresh = true;          // the inner loop of the reference starts with a test of the whole current box
    // steps of a round-robin that starts after position i: how many of the steps 0 .. s-1 fall on list position p
    // (Divisions by ncand: n / ncand == (n * ceil(2^16 / ncand)) >> 16 exactly for 0 <= n < 512 and ncand in [1, 6].  The dividends are a
    //  step of a round, `s` <= SFC_LANES - 1, the steps a round accepts, `accepted` <= SFC_LANES, and those plus a list position < 6: at
    //  most SFC_LANES + 6, and never negative where div_nc / mod_nc see them.  The speculation is one step per lane, so the bound is the
    //  wave's size: asserted below, lest a wider workgroup break the exactness unnoticed.  The compiler's sequence for a division by a
    //  run-time value is ~30 instructions, and a round makes eight of them per lane: more instructions than the slab test they feed.)
    constexpr int SFC_LANES = 64;
    static_assert(SFC_LANES + 6 < 512, "div_nc is exact for dividends below 512 only");
    unsigned magic = (65536u + 5u) / 6u;
    auto div_nc = [&](int n) { return (int)(((unsigned)n * magic) >> 16); };
    auto mod_nc = [&](int n) { return n - div_nc(n) * ncand; };
    auto hits = [&](int s, int p) {
        int t0 = p - i - 1;                                   // in [-ncand, ncand): its residue by one conditional addition
        if (t0 < 0) t0 += ncand;
        return s > t0 ? div_nc(s - t0 - 1) + 1 : 0;
    };
    while (ncand > 0) {
        // lane 0 of a fresh round tests the current box itself; lane l tests step s = l - fresh of this round
        const int s = lane - (fresh ? 1 : 0);
        int c0 = cnt0, c1 = cnt1, c2 = cnt2, c3 = cnt3, c4 = cnt4, c5 = cnt5;
        for (int p = 0; p < ncand; p++) {
            const int axis = (cpack >> (3 * p)) & 7;          // uniform
            const int h = hits(s, p);
            c0 += axis == 0 ? h : 0; c1 += axis == 1 ? h : 0; c2 += axis == 2 ? h : 0;
            c3 += axis == 3 ? h : 0; c4 += axis == 4 ? h : 0; c5 += axis == 5 ? h : 0;
        }
        const int lim = TL - 2;
        c0 = c0 < lim ? c0 : lim; c1 = c1 < lim ? c1 : lim; c2 = c2 < lim ? c2 : lim;
        c3 = c3 < lim ? c3 : lim; c4 = c4 < lim ? c4 : lim; c5 = c5 < lim ? c5 : lim;
        double upd[6];
        upd[0] = T[0 * TL + c0]; upd[1] = T[1 * TL + c1]; upd[2] = T[2 * TL + c2];
        upd[3] = T[3 * TL + c3]; upd[4] = T[4 * TL + c4]; upd[5] = T[5 * TL + c5];
        if (s >= 0) {
            int pos = mod_nc(i + 1 + s);
            const int axis = (cpack >> (3 * pos)) & 7;        // this lane's direction; the slab is [new face, old face]
            if (axis == 0) { upd[3] = upd[0]; upd[0] = T[0 * TL + c0 + 1]; }
            else if (axis == 1) { upd[4] = upd[1]; upd[1] = T[1 * TL + c1 + 1]; }
            else if (axis == 2) { upd[5] = upd[2]; upd[2] = T[2 * TL + c2 + 1]; }
            else if (axis == 3) { upd[0] = upd[3]; upd[3] = T[3 * TL + c3 + 1]; }
            else if (axis == 4) { upd[1] = upd[4]; upd[4] = T[4 * TL + c4 + 1]; }
            else { upd[2] = upd[5]; upd[5] = T[5 * TL + c5 + 1]; }
        }
        const bool fail = sfc_blocked(g, upd) || !sfc_in_boundary(g, upd);
        const unsigned long long fm = __ballot(fail);
        int accepted;                                         // steps of this round that the reference accepts
        if (fm == 0ull) accepted = SFC_LANES - (fresh ? 1 : 0);
        else accepted = (__ffsll((long long)fm) - 1) - (fresh ? 1 : 0);   // -1: the whole-box test itself failed
        if (accepted > 0) {
            for (int p = 0; p < ncand; p++) {
                const int axis = (cpack >> (3 * p)) & 7;
                const int h = hits(accepted, p);
                cnt0 += axis == 0 ? h : 0; cnt1 += axis == 1 ? h : 0; cnt2 += axis == 2 ? h : 0;
                cnt3 += axis == 3 ? h : 0; cnt4 += axis == 4 ? h : 0; cnt5 += axis == 5 ? h : 0;
            }
        }
        if (fm == 0ull) {
            i = mod_nc(i + accepted);                         // position of the last accepted step
            fresh = false;
            continue;
        }
        if (accepted >= 0) i = mod_nc(i + 1 + accepted);      // position of the failing step
        if (i < 0) return 2;
        // drop direction i
        {
            const unsigned lowmask = (1u << (3 * i)) - 1u;
            cpack = (cpack & lowmask) | ((cpack >> (3 * (i + 1))) << (3 * i));
        }
        ncand--;
        magic = ncand > 0 ? (65536u + (unsigned)ncand - 1u) / (unsigned)ncand : 0u;
        if (i > 0) i--;
        else i = ncand - 1;
        fresh = true;
    }
    out[0] = T[0 * TL + cnt0]; out[1] = T[1 * TL + cnt1]; out[2] = T[2 * TL + cnt2];
    out[3] = T[3 * TL + cnt3]; out[4] = T[4 * TL + cnt4]; out[5] = T[5 * TL + cnt5];
    return 0;
}

// one wave per agent; SA: the argument block as the caller holds it (`const SfcArgs`, the kernel's parameter, or KSfcArgs of a batch)
template <class SA>
__device__ __forceinline__ void sfc_agent(SA &a, const int al)
{
    const int lane = threadIdx.x;
    const int qi = a.first + al;
    SfcGrid g;
    g.I = a.integral + (size_t)a.img_of_agent[qi] * (size_t)(a.nx + 1) * (a.ny + 1) * (a.nz + 1);
    g.nx = a.nx; g.ny = a.ny; g.nz = a.nz;
    for (int k = 0; k < 3; k++) { g.kmin[k] = a.key_min[k]; g.wmin[k] = (double)a.world_min[k]; g.wmax[k] = (double)a.world_max[k]; }
    g.rf = a.rf; g.wres = a.wres;
    float *sfc = a.sfc + (size_t)qi * M * 6;
    const float *goal = a.goal + 3 * qi;
    double box[6];
    int rc;
    bool init = a.init_flag[qi] != 0;
    // Both places the seed can come from -- the current position, the end of the previous plan -- and the goal are requested HERE, with the
    // flag that picks the seed: one trip to memory.  (Picked first and fetched then, the seed stood a second trip behind the flag, on a
    // wave that has nothing else to do: the corridor launch of a small swarm is a chain of such trips.)
    // The end of the previous plan is read on EVERY call that has a previous-plan buffer, the first tick and a reset included, where that
    // buffer may hold nothing yet: with `init` set the value is discarded below, never used.
    float s_now[3], s_end[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; k++) s_now[k] = a.state[9 * qi + k];
    if (a.traj_prev != nullptr) {
        const float *t = a.traj_prev + (size_t)qi * NV;
        const int c = (M - 1) * NC + DEG;
        s_end[0] = t[c]; s_end[1] = t[SEGV + c]; s_end[2] = t[2 * SEGV + c];
    }
    const float gl[3] = {goal[0], goal[1], goal[2]};
    if (a.reset_thr > 0.0 && a.planner_seq >= 2) {
        // off the plan (initialTrajPlanningCheck) -> flag_initialize_sfc: the corridor starts again from the current position
        const float *t = a.traj_prev + (size_t)qi * NV + NC;
        const float t1[3] = {t[0], t[SEGV], t[2 * SEGV]};
        if (rule_off_plan(t1, a.state + 9 * qi, a.reset_thr)) init = true;
    }
    float seed[3];
    for (int k = 0; k < 3; k++) seed[k] = init ? s_now[k] : s_end[k];
    extern __shared__ __align__(16) unsigned char sfc_smem[];
    rc = sfc_expand(g, seed, gl, box, reinterpret_cast<double *>(sfc_smem), a.table_len);
    // The shift of the previous boxes reads what it overwrites.  Lane l holds float l of the NEW history: the old values
    // are fetched with one per-lane (vector) load before anything is stored.  (A single lane walking the array reads it
    // through wave-uniform addresses, which the compiler turns into scalar loads; those are not ordered against the
    // vector stores that follow, and a store could overtake the load of the element it replaces.)
    float keep = 0.0f;
    if (!init && lane < (M - 1) * 6) keep = sfc[6 + lane];
    if (rc == 0) {
        const int j = lane % 6;
        const float nb = (float)(j == 0 ? box[0] : j == 1 ? box[1] : j == 2 ? box[2] : j == 3 ? box[3] : j == 4 ? box[4] : box[5]);
        if (init) {
            if (lane < M * 6) sfc[lane] = nb;
        } else if (lane < (M - 1) * 6) {
            sfc[lane] = keep;
        } else if (lane < M * 6) {
            sfc[lane] = nb;
        }
    }
    if (lane == 0) {
        if (rc == 0 && init) a.init_flag[qi] = 0;
        a.err[qi] = rc;
    }
}

__global__ __launch_bounds__(64) void lsc_sfc_kernel(SfcArgs a)
{
    sfc_agent<const SfcArgs>(a, blockIdx.x);
}

// the corridor update of several swarms in one launch (blockIdx.y = swarm, SfcBatch in lsc_kernels.h), each block on its own argument block
__global__ __launch_bounds__(64) void lsc_sfc_batch_kernel(SfcBatch)
{
#if defined(__HIP_DEVICE_COMPILE__)
    KSfcArgs *ka = (KSfcArgs *)__builtin_amdgcn_kernarg_segment_ptr() + blockIdx.y;
#else
    KSfcArgs *ka = nullptr;                                                          // (host pass of the single-source build)
#endif
    if ((int)blockIdx.x >= ka->count) return;
    sfc_agent<KSfcArgs>(*ka, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------
// The per-agent planning kernel
// ---------------------------------------------------------------------------------------------------
constexpr int NB = NCP - 3;   // control points that carry LSC rows: all but (m=0, i<3)   (27 for M = 5)
// Row reduction (reduce_rows): a lane sums all components over a few consecutive rows of one control point's bucket, a second
// step adds the parts of a bucket in order.  Slots = lanes of the first step; their partial sums are staged in LDS that is dead
// at that point: K (NY x KLD doubles, 12 components per slot) before a factorisation, the factorisation's scratch (colbuf, mid2,
// xch: 388 doubles, 3 components per slot: a corrector pass only needs sum v n) in a corrector pass.
constexpr int RSLOT_P = (NY * KLD) / 12, RSLOT_C = 128;
constexpr int AXVALID = AXVALID_3D;  // M = 5: 162 bound + 138 velocity + 114 acceleration rows (src/traj_optimizer.cpp:274-303, 468-525)

// SMALL = the throughput build's variant: what can be recomputed or read from L2 (right-hand sides of the axis rows, the
// constant part of the Hessian entries, the assembly tables) is not kept, the LDS goes to row capacity instead
template <bool SMALL>
struct SmemT {
    // PDIP vectors
    double x[96], dx[96];       // control points (axis-major, 90 used) and their step
    double gx[96];              // x-space gradient: cost + sum a_r v_r
    double gz[96];              // cost + sum a_r z_r  (stationarity residual before projection)
    double y[40], dy[40], rhs[40];
    double W[W_SIZE];           // x-space Hessian weights (see lsc_model.hpp)
    double Tv[NCP * 3];         // per control point: -sum v n over its LSC rows
    double Tz[NCP * 3];         // per control point: -sum z n
    double K[NY * KLD];         // reduced Hessian (lower band); rows of its Cholesky factor after factor()
    double red[2][5][SMALL ? 4 : NWAVE];    // per-wave partials of the block reductions, two banks used in turn (one barrier per reduction); SMALL: four waves
    double colbuf[2][2 * 64];   // column broadcast buffers of the two factorising waves (double-buffered by column parity)
    double mid2[BAND * BAND + 7];   // Schur contribution of the bottom-up sweep to the middle block (original indices); + room for the corrector-pass staging
    double dinv[NY + 1];            // 1 / d of the pivots of K = T D T^T taken top-down (unknown = index), stored by every lane as each is formed
    double dinvb[(NY - BAND) / 2 + 1];   // ... of the pivots of the bottom-up sweep, in ITS order (index q = unknown NY - 1 - q)
    double ok2;                 // pivots of the bottom-up sweep all positive
    double sc[8];               // broadcast scalars
    double gap0;                // complementarity gap at the first iteration of the current start (divergence test)
    // axis rows: slot = type*90 + k*30 + t ; type 0 x<=hi, 1 -x<=-lo, 2/3 +-velocity, 4/5 +-acceleration
    double as_[AXROWS], az[AXROWS], at1[AXROWS], at2[AXROWS], ah[SMALL ? 2 : AXROWS];
    double vlim[3], alim[3];    // right-hand sides of the velocity / acceleration rows (SMALL: ah is computed from these)
    uint32_t amap[AXVALID + 2];   // valid slots, compact: slot | type << 10 | axis k << 13 | t << 15 (decoded by shifts: the row passes visit every row four times an iteration)
    // solver constants addressed per lane (LDS tables instead of ~40 long-lived registers per lane, which the
    // register allocator would otherwise park in scratch for the whole kernel)
    double xtc[SEGV][3];        // x_t = sum xtc[t][j] * y[xgp byte j]   (zero beyond the stencil length)
    double ytc[NY][4];          // gy = sum ytc[g][j] * gx[yop byte j]
    double Qh6[NC * NC];        // 2 w_c Q_base (cost gradient stencil)
    uint32_t xgp[NV];           // three global y indices per variable, one per byte
    uint32_t yop[NY], ypp[NY];  // four x indices (axis-major / point-major) per unknown, one per byte
    unsigned char avalid[SMALL ? 4 : AXROWS];   // (SMALL: the cold start works the validity of a slot out itself)
    // agent constants
    double s0[3][3];            // c_{0,0..2} per axis
    double x0c[SMALL ? 1 : NV]; // the same constants addressed by variable index (k*30 + t, t < 3)  (SMALL: read from s0)
    double lo[3][M], hi[3][M];  // bounds per axis and segment (world box, intersected with the SFC)
    double goal[3];
    double reachL[3][28], reachU[3][28];   // per axis: bounds of c_{m,i} - c_{0,2} after K = 5m+i-2 steps (phase B pruning)
    float pinit[NV];            // own initial trajectory (float32)
    int cnt[32];                // rows per control-point bucket
    int offs[32];               // exclusive prefix of cnt over the 27 buckets
    uint32_t offcnt[32];        // offs | cnt << 16 per bucket (LDS pass: both below 65536), one load per reduction unit
    int wcnt[SMALL ? 4 : NWAVE][32];
    // row reduction: slots = (bucket, part) pairs, one lane each; two granularities (predictor / corrector staging sizes differ)
    uint32_t slotP[RSLOT_P], slotC[RSLOT_C];   // first row | rows << 16 | bucket << 24
    unsigned short soffP[NB + 1], soffC[NB + 1];   // first slot of every bucket (+ total)
    double cullB[M];            // phase B pre-cull: per segment max_i(|c_{0,2} - p_{m,i}| + reach radius of c_{m,i})
    double cullA[2];            // obstacle-level cull: rho_a = max |c_{0,2} - p| over the own points, max_m cullB[m]
    int cullc[NWAVE + 1];       // survivors of the pre-cull per wave (compaction)
    int rpl[2];                 // rows per slot of the row reduction (predictor / corrector granularity)
    int ntmp;                   // rows appended in phase B (arrival order), listfull: the pre-cull list overflowed
    int listfull;
    int tseg;                   // terminal segments
    int flag;                   // capacity overflow
    int gen;                    // alternate-mode QP: lsc_general_kernel solves this agent
    int nact;                   // active LSC rows
    int itmp;                   // argmin scratch of the goal stage
    float goalf[3];             // current goal (float32, as agent.current_goal_position)
    alignas(8) uint32_t dyn[2]; // dynamic part starts here: terms, entry table, kconst, LSC rows, row map
};
using Smem = SmemT<false>;

// Row `type` of variable (k, t) applied to x: bound (x_t), velocity (x_{t+1} - x_t) or acceleration (x_{t+2} - 2 x_{t+1} + x_t)
// difference, odd types negated.  Branch-free on purpose: the lanes of a wave hold rows of all six types, and a switch runs
// every case one after the other; three loads (x has room behind its 90 entries) and three multiply-adds with coefficients
// selected by the type cost less than one of its cases did.
__device__ __forceinline__ double ax_row(const double *x, int type, int k, int t)
{
    const double *xk = x + k * SEGV + t;
    const int kind = type >> 1;                                       // 0 bound, 1 velocity, 2 acceleration
    const double a0 = kind == 1 ? -1.0 : 1.0, a1 = kind == 0 ? 0.0 : (kind == 1 ? 1.0 : -2.0), a2 = kind == 2 ? 1.0 : 0.0;
    const double v = fma(a2, xk[2], fma(a1, xk[1], a0 * xk[0]));
    return (type & 1) ? -v : v;
}

// the same from three loaded values (the row passes load everything a row needs in one batch, see LSC_PIN)
__device__ __forceinline__ double ax_row3(double x0, double x1, double x2, int type)
{
    const int kind = type >> 1;
    const double a0 = kind == 1 ? -1.0 : 1.0, a1 = kind == 0 ? 0.0 : (kind == 1 ? 1.0 : -2.0), a2 = kind == 2 ? 1.0 : 0.0;
    const double v = fma(a2, x2, fma(a1, x1, a0 * x0));
    return (type & 1) ? -v : v;
}
// All operands in registers HERE: the loads that produce them are issued together ahead of this point and waited for once.  Left to
// itself the scheduler puts every load directly in front of its first use -- four to five LDS round trips per row in the row passes.
#define LSC_PIN(...) asm volatile("" : __VA_ARGS__)
#define PV(x) "+v"(x)

// value of lane L (compile-time) broadcast to the wave: two v_readlane_b32, no LDS round trip
template <int L>
__device__ __forceinline__ double bcast_lane(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, L);
    hi = __builtin_amdgcn_readlane(hi, L);
    return __hiloint2double(hi, lo);
}

// 1/sqrt(d): hardware seed (v_rsq_f64) + two Newton steps -> full double precision, no sqrt / divide sequence
__device__ __forceinline__ double rsqrt_nr(double d)
{
    double y = __builtin_amdgcn_rsq(d);
    double e = fma(-d * y, y, 1.0);
    y = fma(0.5 * y, e, y);
    e = fma(-d * y, y, 1.0);
    y = fma(0.5 * y, e, y);
    return y;
}

// Right-looking banded LDL^T of the 39x39 reduced Hessian (K = M D M^T, M unit lower triangular, D = diag(d)) in the
// registers of wave 0: lane i owns row i (column index = register index).  No square roots: the dependency chain of
// a column is  readlane(d_J) -> 1/d_J (v_rcp_f64 + 1 Newton step) -> u = row[J]/d_J -> one fma into the next pivot.
// Column J's (unscaled) entries reach the other lanes two ways:
//   * k = J+1 .. J+3 (needed by the next three pivots): v_readlane, issued before the reciprocal is known;
//   * k = J+4 .. J+11: the column is published once in LDS and read back as broadcast loads; those loads are issued
//     at the start of step J and their updates are applied during step J+2, so the LDS latency is hidden behind two
//     pivot chains wherever the instruction scheduler places the uses.
constexpr int CHOL_NEAR = 3;
__device__ __forceinline__ double rcp_nr(double d)
{
    // v_rcp_f64 seed (~2^-26 relative) + one Newton step -> ~2^-51: as accurate as the factorisation needs (the compiler's
    // correctly rounded division spends a second step and a fix-up on the last half ulp)
    double y = __builtin_amdgcn_rcp(d);
    double e = fma(-d, y, 1.0);
    y = fma(y, e, y);
    return y;
}
template <int J, int JEND>
__device__ __forceinline__ void chol_step(double (&row)[NY], double *colbuf, double *dinv_out, int lane, int &npos,
                                          double u_p1, const double (&pend_p1)[BAND], double u_p2, const double (&pend_p2)[BAND])
{
    constexpr int K1 = (J + BAND) < (NY - 1) ? (J + BAND) : (NY - 1);
    const double cj = row[J];             // A[i][J] after the updates of columns < J (lane J: the pivot d_J)
    // publish the column and issue the loads for its far entries first: nothing depends on them until step J+2
    double nxt[BAND];
#pragma unroll
    for (int q = 0; q < BAND; q++) nxt[q] = 0.0;
    if constexpr (J + 1 + CHOL_NEAR <= K1) {
        double *buf = colbuf + (J & 1) * 64;
        buf[lane] = cj;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < BAND; q++) {
            const int k = J + 1 + CHOL_NEAR + q;
            if (k <= K1) nxt[q] = buf[k];
        }
    }
    // ---- critical part: pivot J and the updates the next three pivots depend on
    const double dj = bcast_lane<J>(cj);
    const double s1 = bcast_lane<(J + 1 < NY ? J + 1 : 0)>(cj);
    const double s2 = bcast_lane<(J + 2 < NY ? J + 2 : 0)>(cj);
    const double s3 = bcast_lane<(J + 3 < NY ? J + 3 : 0)>(cj);
    npos += dj > 0.0 ? 1 : 0;             // (a count, not a flag: the chain of ANDs behind a flag is kept in scalar pairs to the end of the sweep)
    const double r = rcp_nr(dj);          // 1 / d_J, uniform over the wave: every lane stores the same word (selecting lane J's copy at the end
    dinv_out[J] = r;                      // of the sweep costs two restored predicate words and two selects per pivot)
    const double u = cj * r;              // M[i][J] = A[i][J] / d_J  (unit-diagonal factor entry)
    if constexpr (J + 1 <= K1) row[J + 1] = fma(-u, s1, row[J + 1]);
    if constexpr (J + 2 <= K1) row[J + 2] = fma(-u, s2, row[J + 2]);
    if constexpr (J + 3 <= K1) row[J + 3] = fma(-u, s3, row[J + 3]);
    // ---- deferred part of column J-2 (its LDS loads were issued two steps ago)
    if constexpr (J >= 2) {
        constexpr int P = J - 2;
        constexpr int PK1 = (P + BAND) < (NY - 1) ? (P + BAND) : (NY - 1);
#pragma unroll
        for (int q = 0; q < BAND; q++) {
            const int k = P + 1 + CHOL_NEAR + q;
            if (k <= PK1) row[k] = fma(-u_p2, pend_p2[q], row[k]);
        }
    }
    row[J] = u;
    if constexpr (J + 1 < JEND) chol_step<J + 1, JEND>(row, colbuf, dinv_out, lane, npos, u, nxt, u_p1, pend_p1);
    else {
        // end of this range of pivots: apply the far-column updates of the last two columns that are still deferred
        if constexpr (J >= 1) {
            constexpr int P = J - 1;
            constexpr int PK1 = (P + BAND) < (NY - 1) ? (P + BAND) : (NY - 1);
#pragma unroll
            for (int q = 0; q < BAND; q++) {
                const int k = P + 1 + CHOL_NEAR + q;
                if (k <= PK1) row[k] = fma(-u_p1, pend_p1[q], row[k]);
            }
        }
#pragma unroll
        for (int q = 0; q < BAND; q++) {
            const int k = J + 1 + CHOL_NEAR + q;
            if (k <= K1) row[k] = fma(-u, nxt[q], row[k]);
        }
    }
}

// Twisted ("burn at both ends") factorisation: wave 0 eliminates columns 0..13 top-down, wave 1 columns 38..25
// bottom-up (the same code on the index-reversed matrix), both Schur complements land on the 11x11 middle block
// [14, 25) which wave 0 then factorises.  K = T D T^T with T unit lower triangular in its first 25 columns and unit
// upper triangular in its last 14; the dependent chain is 14 + 11 pivots instead of 39.  The substitutions use the
// same split: 14 steps from both ends in parallel, 11 + 10 in the middle, 13 steps back out in parallel.
constexpr int TW_A = (NY - BAND + 1) / 2; // pivots taken from the top ...            (14 for NY = 39, 10 for NY = 30)
constexpr int TW_B = NY - BAND - TW_A;    // ... and from the bottom (the same, or one less)  (14,             9)
constexpr int TW_M1 = NY - TW_B;          // middle block = [TW_A, TW_M1)
static_assert(TW_M1 - TW_A == BAND, "the middle block must absorb exactly one bandwidth");

template <int J, int JEND>
__device__ __forceinline__ void fwd_steps(const double (&rowS)[TW_M1], double &b)
{
    const double bj = bcast_lane<J>(b);
    b = fma(-rowS[J], bj, b);
    if constexpr (J + 1 < JEND) fwd_steps<J + 1, JEND>(rowS, b);
}
// backward steps I = HI .. LO: lane i < I gets  b_i -= c[I - LO] * x_I  (c: column entries T[I][lane], zero where absent)
template <int I, int LO, int CNT>
__device__ __forceinline__ void bwd_steps(const double (&c)[CNT], double &b)
{
    const double xi = bcast_lane<I>(b);
    b = fma(-c[I - LO], xi, b);
    if constexpr (I > LO) bwd_steps<I - 1, LO, CNT>(c, b);
}

// Values that must be in registers HERE: an empty volatile statement that names them all.  (The compiler otherwise sinks each
// load of a "condition ? loaded value : 0" into a branch of its own -- exec mask, load, wait, restore -- and the loads of one
// group, which are independent, are served one LDS latency after the other.)
#define LSC_P(a, i) "+v"(a[i])
__device__ __forceinline__ void pin_values(double (&a)[4])
{
    asm volatile("" : LSC_P(a, 0), LSC_P(a, 1), LSC_P(a, 2), LSC_P(a, 3));
}
__device__ __forceinline__ void pin_values(double (&a)[8])
{
    asm volatile("" : LSC_P(a, 0), LSC_P(a, 1), LSC_P(a, 2), LSC_P(a, 3), LSC_P(a, 4), LSC_P(a, 5), LSC_P(a, 6), LSC_P(a, 7));
}
__device__ __forceinline__ void pin_values(double (&a)[9])
{
    asm volatile("" : LSC_P(a, 0), LSC_P(a, 1), LSC_P(a, 2), LSC_P(a, 3), LSC_P(a, 4), LSC_P(a, 5), LSC_P(a, 6), LSC_P(a, 7), LSC_P(a, 8));
}
__device__ __forceinline__ void pin_values(double (&a)[10])
{
    asm volatile("" : LSC_P(a, 0), LSC_P(a, 1), LSC_P(a, 2), LSC_P(a, 3), LSC_P(a, 4), LSC_P(a, 5), LSC_P(a, 6), LSC_P(a, 7), LSC_P(a, 8), LSC_P(a, 9));
}
__device__ __forceinline__ void pin_values(double (&a)[11])
{
    asm volatile("" : LSC_P(a, 0), LSC_P(a, 1), LSC_P(a, 2), LSC_P(a, 3), LSC_P(a, 4), LSC_P(a, 5), LSC_P(a, 6), LSC_P(a, 7), LSC_P(a, 8), LSC_P(a, 9),
                 LSC_P(a, 10));
}
__device__ __forceinline__ void pin_values(double (&a)[12])
{
    asm volatile("" : LSC_P(a, 0), LSC_P(a, 1), LSC_P(a, 2), LSC_P(a, 3), LSC_P(a, 4), LSC_P(a, 5), LSC_P(a, 6), LSC_P(a, 7), LSC_P(a, 8), LSC_P(a, 9), LSC_P(a, 10), LSC_P(a, 11));
}
__device__ __forceinline__ void pin_values(double (&a)[13])
{
    asm volatile("" : LSC_P(a, 0), LSC_P(a, 1), LSC_P(a, 2), LSC_P(a, 3), LSC_P(a, 4), LSC_P(a, 5), LSC_P(a, 6), LSC_P(a, 7), LSC_P(a, 8), LSC_P(a, 9),
                 LSC_P(a, 10), LSC_P(a, 11), LSC_P(a, 12));
}
__device__ __forceinline__ void pin_values(double (&a)[14])
{
    asm volatile("" : LSC_P(a, 0), LSC_P(a, 1), LSC_P(a, 2), LSC_P(a, 3), LSC_P(a, 4), LSC_P(a, 5), LSC_P(a, 6), LSC_P(a, 7), LSC_P(a, 8), LSC_P(a, 9),
                 LSC_P(a, 10), LSC_P(a, 11), LSC_P(a, 12), LSC_P(a, 13));
}
#undef LSC_P

// phase stamps (PROF variant only): cycles of lane 0 spent per phase, accumulated per agent
enum { PH_SETUP = 0, PH_LSC, PH_INIT, PH_P1, PH_REDUCE, PH_ASSEMBLE, PH_FACTOR, PH_SOLVE, PH_P2, PH_P3, PH_P45, PH_OUT,
       PH_RED_BUCKETS /* part of PH_REDUCE: the LSC-bucket sums of wave 0, before the barrier */, PH_RED_GATHER /* the axis-row gather, clocked by the last lane */,
       PH_SPARE0, PH_SPARE1, PH_COUNT };
static_assert(PH_COUNT == PROF_PHASES, "lsc_phase_profile copies PROF_PHASES counters per agent");


// One agent's replan on one 512-lane workgroup.
//   SPILL = false : the LSC rows live in LDS (at most a.cap rows per control point); an agent with more rows than that
//                   is flagged LSC_STATUS_CAPACITY_K and left to the second pass
//   SPILL = true  : the row arrays live in this workgroup's HBM workspace `ws`, sized for all 27 (N-1) rows the
//                   reference adds (src/traj_optimizer.cpp:437-466) -- same code, same arithmetic, no capacity limit
//   ALT = true    : the build with the alternate-mode hooks (disturbance checks, hand-over to lsc_general_kernel); kept
//                   out of the default instantiation so that the fast path's register allocation is untouched by them
//   NTT           : lanes of the workgroup -- 512 (8 waves, one workgroup per CU: the latency build) or 256 (4 waves, two
//                   workgroups per CU when the LDS request allows it: the throughput build for swarms larger than the chip)
//   DIM2          : planar world (world/dimension == 2): a compile-time switch, because as a run-time flag it cost the non-planar
//                   kernel 1.5 % (measured: six missions 184.2 -> 186.9 ms of kernel time with the flag, 184.x without)
//   ArgsT         : the argument block as the caller holds it -- `const PlanArgs` (the kernel's by-value parameter) or KArgs (a block
//                   of a batch launch, read where it lies in the kernarg segment)
//   SOLVER        : 0 the interior point alone; 1 a dual active-set solve first (gi_solve below: Goldfarb-Idnani from the unconstrained
//                   optimum), the interior point only when that gives up
//   OBS           : the mission's dynamic obstacles (a.obs: K non-cooperating moving spheres) follow the other N - 1 agents in every agent's
//                   obstacle list: obstacle index oi < N - 1 is agent qj = oi + (oi >= qi) as ever, oi >= N - 1 gives qj >= N and qj - N is the
//                   dynamic obstacle.  Only phase B sees them (goal planning, the retreat rule and the terminal segments walk agents only:
//                   traj_planner.cpp:553); a compile-time switch, so that no other instantiation carries any of it
// Returns whether phase A handed the agent over to the general solver (status LSC_STATUS_GENERAL_K; ALT builds only), uniform.
template <bool PROF, bool SPILL, bool ALT = false, int NTT = 512, bool DIM2 = false, class ArgsT = const PlanArgs, int SOLVER = 0, bool OBS = false>
__device__ __forceinline__ bool plan_agent(ArgsT &a, const int al, unsigned char *smem_raw, unsigned char *ws)
{
    static_assert(SOLVER == 0 || !SPILL, "the active-set solve keeps its rows in LDS");
    static_assert(!OBS || (!DIM2 && !PROF && NTT == 512), "dynamic obstacles: the 3-D latency kernels and the second pass only");
    static_assert(!(OBS && ALT && SPILL), "dynamic obstacles with the alternate-mode hooks: the latency kernel only");
    constexpr int WS_FEW_ROWS = 200;
    constexpr int NT = NTT;             // shadow the namespace-level constants (those size the LDS arrays: maxima)
    constexpr int NWAVE = NTT / 64;
    // cmap entry = row slot | control point << CMAP_SHIFT (HBM variant: 24 bits of slot, 27 (N-1) slots fit for any N)
    constexpr int CMAP_SHIFT = SPILL ? 24 : 16;
    constexpr uint32_t CMAP_MASK = (1u << CMAP_SHIFT) - 1u;
    long long t_last = 0;
    long long t_acc[PH_COUNT];
    if constexpr (PROF) {
#pragma unroll
        for (int i = 0; i < PH_COUNT; i++) t_acc[i] = 0;
        t_last = wall_clock64();
    }
    auto stamp = [&](int ph) {
        if constexpr (PROF) {
            long long now = wall_clock64();
            t_acc[ph] += now - t_last;
            t_last = now;
        }
    };
    constexpr bool TABLES_IN_LDS = NTT != 256;
    SmemT<!TABLES_IN_LDS> &S = *reinterpret_cast<SmemT<!TABLES_IN_LDS> *>(smem_raw);
    const Model &md = *a.model;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qi = a.first + al;
    const int N = a.N;
    int n_obs = N - 1;
    // (the block of dynamic obstacles: its address and K are the same in all lanes, and SAID to be)
    const ObsBlock *ob = nullptr;
    if constexpr (OBS) {
        ob = uniform_ptr(a.obs);
        n_obs += __builtin_amdgcn_readfirstlane(ob->K);
    }
    // Row capacity of this pass.  Rows are stored COMPACTLY, sorted by control point (bucket b occupies
    // [offs[b], offs[b] + cnt[b])), so the capacity is a total, not a per-bucket limit: LDS pass a.cap rows, HBM pass all
    // 27 (N-1) rows the reference can add.
    const int R = SPILL ? NB * (n_obs > 1 ? n_obs : 1) : a.cap;
    const int n_terms = md.n_terms, n_entries = md.n_entries;
    // axis rows that exist: 414, or 276 in a planar world (no z rows: `for (k < dim)`, src/traj_optimizer.cpp:274, 469)
    constexpr int n_ax = DIM2 ? AXVALID_2D : AXVALID_3D;
    constexpr bool dim2 = DIM2;

    // dynamic LDS carve-up.  The throughput build leaves the (agent-independent, 9 KB) assembly tables in HBM/L2 -- its two
    // workgroups per CU hide that latency -- and spends the LDS on row capacity instead.
    const uint32_t *terms, *ent;
    double *kconst;
    // (SOLVER == 1: everything only the interior point needs -- these tables, the constant part of the Hessian entries, the slot tables of the
    //  row reduction, its zeroed arrays -- is set up where the active-set solve hands over to it, once in ~2 000 agent-replans: ip_late_setup)
    if constexpr (TABLES_IN_LDS) {
        uint32_t *lt = S.dyn;                                       // [n_terms]
        uint32_t *le = lt + ((n_terms + 1) & ~1);                   // [n_entries+1][2] : (gi<<16|gj), first term
        if constexpr (SOLVER != 1) {
            for (int i = tid; i < n_terms; i += NT) lt[i] = a.terms[i];
            for (int i = tid; i < 2 * n_entries + 2; i += NT) le[i] = a.entries[i];
        }
        terms = lt; ent = le;
        kconst = reinterpret_cast<double *>(le + 2 * n_entries + 2);
    } else {
        // (round 5: the constant part of the entries IS kept -- 3.2 KB --: recomputing it in every assembly, with its index divisions and
        //  its loads of the cost Hessian from L2, was half of what the assembly cost more here than in the latency build)
        terms = a.terms; ent = a.entries;
        kconst = reinterpret_cast<double *>(S.dyn);
    }
    double *rowbase;
    if constexpr (SPILL) rowbase = reinterpret_cast<double *>(ws);
    else rowbase = kconst + n_entries;
    double *__restrict__ rrhs = rowbase;
    double *__restrict__ rs = rrhs + R;
    double *__restrict__ rz = rs + R;
    double *__restrict__ rt1 = rz + R;
    double *__restrict__ rt2 = rt1 + R;
    float *__restrict__ rn = reinterpret_cast<float *>(rt2 + R);     // [3][R]
    uint32_t *__restrict__ cmap = reinterpret_cast<uint32_t *>(rn + 3 * R);  // row map: slot | cp << CMAP_SHIFT
#ifdef LSC_POISON_LDS
    // debugging aid (not built into the product): every byte of the workgroup's LDS starts as 0xff -- NaN as a double, -1 as an
    // index -- so that a read of something that was never written shows up as a failed plan or a fault instead of once in a while
    if constexpr (!SPILL) {
        uint32_t *pw = reinterpret_cast<uint32_t *>(smem_raw), *pe = cmap + R;
        const int skip = TABLES_IN_LDS ? (int)(reinterpret_cast<uint32_t *>(rowbase) - pw) : 0;      // (the tables were copied in above)
        for (uint32_t *q = pw + tid; q < pe; q += NT) {
            const int i = (int)(q - pw);
            if (i >= (int)(reinterpret_cast<uint32_t *>(S.dyn) - pw) && i < skip) continue;
            *q = 0xffffffffu;
        }
        __syncthreads();
    }
#endif
    // phase B scratch, aliased onto arrays that are first written later: rows in arrival order (rs .. rt2, 32 B per row,
    // written by phase C's start) and the pre-cull's unit list (rn .. cmap, written by the scatter that ends phase B)
    struct TmpRow { double rhs; float nx, ny, nz; uint32_t cp_pos; };
    static_assert(sizeof(TmpRow) <= 4 * sizeof(double), "a temporary row fits the (rs, rz, rt1, rt2) slot of a row");
    TmpRow *tmp_rows = reinterpret_cast<TmpRow *>(rs);

    // Small swarms build their rows one wave per segment and store them straight to their final slots (phase B): nothing is left to scatter.
    // Decided ONCE, here: at most 64 obstacles, the context not held to the generic pass, no list of units given.  (A list exists only for
    // swarms of NEIGH_MIN_AGENTS and more -- a.nv --, and the in-kernel cull needs more than NT units: 64 obstacles have 64 M <= NT.)
    // With `placed` the waves also take ROLES for phases A and B -- the GJK of a small swarm runs on waves 0 .. M-1 and reads nothing of the
    // planned goal, so the goal is planned beside it:
    //   waves 0 .. M-1  (segment waves)  state constants and reach boxes, then straight into the GJK of their segment
    //   wave NWAVE-1    (goal wave)      the scan over the other agents, lane = agent: disturbance checks in front of the first barrier (S.gen is
    //                                    all phase B needs of it), argmin, goal, terminal segments and box bounds beside the GJK, by wave operations
    //   waves M .. NWAVE-2 (copy waves)  the agent-independent tables of the solver, beside the GJK
    // Barriers per role, the same four for every wave up to the solve (no wave waits for another anywhere else):
    //   (1) end of phase A: pinit, s0, x0c, vlim, alim, cnt, gen published    -- every role arrives with only its loads of the top behind it
    //   (2) reach boxes published (written by waves 0 and 1 between (1) and (2); goal and copy waves pass straight through)
    //   (3) in front of the row placement: wcnt of the segment waves; goalf, goal, tseg, lo, hi of the goal wave; the copy waves' tables
    //   (4) rows placed, offsets and counts published
    constexpr bool SEG_WAVES = !SPILL && NTT == 512 && NWAVE >= M;
    static_assert(!SEG_WAVES || (64 * M <= NTT && NWAVE >= M + 2), "a goal wave and a copy wave beside the segment waves; 64 obstacles stay below the cull's threshold");
    bool placed = false;
    // (the same in all lanes, and SAID to be: behind a branch the compiler takes for divergent, what one role holds would stay live -- and go to
    //  scratch -- across the code of the others)
    if constexpr (SEG_WAVES) placed = __builtin_amdgcn_readfirstlane((!a.generic_lsc_build && a.nv == nullptr && n_obs <= 64) ? 1 : 0) != 0;
    const bool roles = SEG_WAVES && placed;
    const int role_wave = __builtin_amdgcn_readfirstlane(wave);
    const bool goal_wave = roles && role_wave == NWAVE - 1;
    constexpr int COPY_T0 = M * 64, COPY_NT = SEG_WAVES ? (NWAVE - 1 - M) * 64 : 64;      // the copy waves' first lane and their lanes
    // what the goal wave carries from its scan (phase A) to the argmin (phase B): this lane's closest candidate, its index and its position
    double gw_best = 1e9, gw_vnom = 0.0;
    int gw_bq = 0x7fffffff;
    float gw_opos[3] = {0.f, 0.f, 0.f};
    int gw_T = 1;                       // its number of terminal segments (SOLVER == 1: in every lane)

    // ------------------------------------------------------------------ phase A: agent constants
    if (tid < 32) S.cnt[tid] = 0;
    if (tid == 0) { S.flag = 0; S.ntmp = 0; }
    if (SOLVER == 1 && tid == 0) S.sc[0] = 0.0;      // (the code of the active-set solve's last step, read at the top of every round: none yet)
    const float dtf = (float)md.dt;
    // What goal planning reads of the other agents (lane = agent) is requested HERE, at the top of the kernel: position, desired goal, three points of its previous plan,
    // its disturbance flag -- one trip to HBM for the checks and the priority rule together
    struct ScanIn { float s[3], g[3], tl[3], tf[3], t1[3]; int ev; };
    auto scan_load = [&](int qj) {
        ScanIn r;
        const float *sp = a.state + 9 * qj, *gp = a.goal + 3 * qj, *pt = a.traj_prev + (size_t)qj * NV;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            r.s[k] = sp[k]; r.g[k] = gp[k];
            r.tl[k] = pt[k * SEGV + (M - 1) * NC + DEG]; r.tf[k] = pt[k * SEGV + DEG]; r.t1[k] = pt[k * SEGV + NC];
        }
        r.ev = a.ever ? (int)a.ever[qj] : 0;
        return r;
    };
    // Large swarms (lsc_neigh.hip): the agents within priority_dist_threshold of this one -- all the priority rule can act on -- come as a short
    // list, and "somebody is off its plan" as one bit of its count: no walk over all N agents (at 1024 agents four rounds of 64-byte loads per
    // lane, at 8192 thirty-two).  n_pc < 0: no such information, everybody is scanned as in small swarms.
    // (every value read through the view is the same for all lanes, and SAID to be: loaded by vector instructions they would sit in vector
    //  registers across the phases -- the production instantiations went from no scratch to 12 bytes per lane)
    const NeighView *const nv = a.nv;
    const int pc_word = nv ? __builtin_amdgcn_readfirstlane(nv->pcnt[qi]) : -1;
    const int n_pc = pc_word >= 0 ? (pc_word & 0xffff) : -1;
    const bool swarm_slack = pc_word >= 0 && ((pc_word >> 30) & 1) != 0;
    const unsigned short *const plist = nv ? uniform_ptr(nv->plist) + (size_t)qi * __builtin_amdgcn_readfirstlane(nv->pcap) : nullptr;
    ScanIn sc0;
    // (roles: the scan is the goal wave's alone, lane = agent; no other wave requests anything for it)
    if (goal_wave) gw_vnom = a.vnom[qi];
    if (a.goal_mode == 1 && goal_wave) sc0 = scan_load(lane < N ? lane : 0);
    else if (a.goal_mode == 1 && !roles) sc0 =scan_load(n_pc >= 0 ? (tid < n_pc ? (int)plist[tid] : qi) : (tid < N ? tid : 0));
    else {
#pragma unroll
        for (int k = 0; k < 3; k++) sc0.s[k] = sc0.g[k] = sc0.tl[k] = sc0.tf[k] = sc0.t1[k] = 0.f;
        sc0.ev = 0;
    }
    if (tid < NV) {
        const int k = tid / SEGV, c = tid % SEGV, m = c / NC, i = c % NC;
        S.pinit[tid] = rule_initial_point(a.state + 9 * qi, a.traj_prev + (size_t)qi * NV + k * SEGV, k, m, i, a.planner_seq, false, dtf);
        // (the branch-free row evaluation, ax_row, reads up to two entries behind the last variable with coefficient zero:
        // they must be numbers)
        if (tid < 6) { S.x[NV + tid] = 0.0; S.dx[NV + tid] = 0.0; }
    }
    // ---- disturbance checks (rule_off_plan): an agent off its plan is "disturbed"; every agent then
    // keeps slack variables on its rows against that agent for the rest of the mission (obs_slack_indices only grows),
    // which is a QP of another shape: the swarm switches to lsc_general_kernel (a.ever = the persistent per-agent flag).
    auto off_plan = [&](int q) {
        const float *t = a.traj_prev + (size_t)q * NV + NC;
        const float t1[3] = {t[0], t[SEGV], t[2 * SEGV]};
        return rule_off_plan(t1, a.state + 9 * q, a.reset_thr);
    };
    const bool checks = ALT && a.reset_thr > 0.0 && a.planner_seq >= 2 && a.planner_mode == 0 && a.ever != nullptr;
    bool own_now = false, own_slack = false;
    if (tid == 0 && !roles) S.gen = ALT ? a.general_all : 0;      // (roles: the goal wave is its only writer)
    // (with prior_based goals the pass over the other agents below does these checks on its way: one round trip to the states instead of
    //  two, one barrier less)
    int any_slack = 0;
    if (checks) {
        own_now = off_plan(qi);
        own_slack = own_now || a.ever[qi] != 0;
        any_slack = own_slack ? 1 : 0;
        if (a.goal_mode != 1 && !roles) {
            if (n_pc >= 0) any_slack |= swarm_slack ? 1 : 0;      // (checked once per agent by the build kernel of the neighbour lists, flags set there)
            else for (int qj = tid; qj < N; qj += NT) {
                const bool nw = off_plan(qj);
                if (nw) a.ever[qj] = 1;
                any_slack |= (nw || a.ever[qj] != 0) ? 1 : 0;
            }
            __syncthreads();              // S.gen was initialised by lane 0 above
            if (any_slack) S.gen = 1;     // every writer stores the same value; read after the next barrier
        }
    }
    const bool rest = ALT && (own_now || a.planner_mode == 1);   // own initial trajectory = current position (reset, or BVC)
    // ---- goal planning (TrajPlanner::goalPlanning, src/traj_planner.cpp:477-538)
    //   static      : current goal = the goal input
    //   prior_based : goalPlanningWithPriority (:540-608) on a map without a distance field.  There the grid A*
    //                 (src/grid_based_planner.cpp) has no observable effect: its path only feeds findLOSFreeGoal
    //                 (:350-407), whose line-of-sight test passes for every point when there are neither static
    //                 obstacles nor a distmap, so the result is the desired goal clamped to goal_radius from the end of
    //                 the initial trajectory -- unless a higher-priority agent is closer than priority_dist_threshold.
    if (roles) {
        // ---- wave roles, in front of barrier (1): only what does not depend on the goal.  State constants and limits as on the generic
        // path behind the goal's barrier below; vmax / amax travel with the loads of the top, not behind a barrier.
        if (tid < 3) {
            const int k = tid;
            const float *s = a.state + 9 * qi;
            double c0, c1, c2;
            rule_state_constants(s[k], s[3 + k], s[6 + k], md.hv_scale, md.ha_scale, dim2 && k == 2, md.z2d, c0, c1, c2);
            S.s0[k][0] = c0; S.s0[k][1] = c1; S.s0[k][2] = c2;
            if constexpr (TABLES_IN_LDS) { S.x0c[k * SEGV] = c0; S.x0c[k * SEGV + 1] = c1; S.x0c[k * SEGV + 2] = c2; }
            S.vlim[k] = a.vmax[3 * qi + k] * md.hv_scale; S.alim[k] = a.amax[3 * qi + k] * md.ha_scale;
        }
        if (goal_wave) {
            // The scan of the generic path below, lane = agent (a second round for agent 64 of a 65-agent swarm); the disturbance checks ride on
            // it.  What is kept for the argmin behind barrier (2) is this lane's closest candidate -- a strict minimum, so the lower index of a
            // lane's two rounds wins a tie -- and ITS position as fetched here: the retreat reads it from the lane that holds it.
            const float *pos = a.state + 9 * qi;
            const float *goal_i = a.goal + 3 * qi;
            if (a.goal_mode == 1) {
                const double dist_to_goal = rule_distf(pos, goal_i);
                for (int qj = lane; qj < N; qj += 64) {
                    const ScanIn in = qj < 64 ? sc0 : scan_load(qj);      // (first round: fetched at the top of the kernel)
                    bool slack_j = false;
                    if (checks) {
                        const bool nw = rule_off_plan(in.t1, in.s, a.reset_thr);      // (on the fetched values)
                        if (nw) a.ever[qj] = 1;
                        slack_j = nw || in.ev != 0;
                        any_slack |= slack_j ? 1 : 0;
                    }
                    if (qj == qi) continue;
                    if (checks && (own_slack || slack_j)) continue;   // slack obstacle: no retreat candidate (:548-551)
                    double dist_to_obs;
                    if (!rule_has_priority(pos, dist_to_goal, in.s, in.g, in.tl, in.tf, a.goal_threshold, dist_to_obs)) continue;
                    if (dist_to_obs < gw_best) { gw_best = dist_to_obs; gw_bq = qj; gw_opos[0] = in.s[0]; gw_opos[1] = in.s[1]; gw_opos[2] = in.s[2]; }
                }
            } else if (checks) {
                for (int qj = lane; qj < N; qj += 64) {
                    const bool nw = off_plan(qj);
                    if (nw) a.ever[qj] = 1;
                    any_slack |= (nw || a.ever[qj] != 0) ? 1 : 0;
                }
            }
            // S.gen, all phase B needs of the scan: one writer, read behind barrier (1)
            const bool flagged = checks && __ballot(any_slack != 0) != 0ull;
            if (lane == 0) S.gen = flagged ? 1 : (ALT ? a.general_all : 0);
        }
    } else if (a.goal_mode == 1) {
        const float *pos = a.state + 9 * qi;
        const float *goal_i = a.goal + 3 * qi;
        const double dist_to_goal = rule_distf(pos, goal_i);
        const int cl = (M - 1) * NC + DEG;             // control point [M-1][n]
        double best = 1e9;
        int bq = 0x7fffffff;
        bool first_round = true;
        const int n_scan = n_pc >= 0 ? n_pc : N;
        if (checks && n_pc >= 0) any_slack |= swarm_slack ? 1 : 0;
        for (int sj = tid; sj < n_scan; sj += NT) {
            const int qj = n_pc >= 0 ? (int)plist[sj] : sj;
            const ScanIn in = first_round ? sc0 : scan_load(qj);      // (first round: fetched at the top of the kernel)
            first_round = false;
            bool slack_j = false;
            if (checks) {
                const bool nw = rule_off_plan(in.t1, in.s, a.reset_thr);      // (on the fetched values)
                if (nw) a.ever[qj] = 1;
                slack_j = nw || in.ev != 0;
                any_slack |= slack_j ? 1 : 0;
            }
            if (qj == qi) continue;
            if (checks && (own_slack || slack_j)) continue;   // slack obstacle: no retreat candidate (:548-551)
            // (in.tl, in.tf: obs_prev_trajs, the unshifted previous plan -- its last and its sixth control point)
            double dist_to_obs;
            if (!rule_has_priority(pos, dist_to_goal, in.s, in.g, in.tl, in.tf, a.goal_threshold, dist_to_obs)) continue;
            if (dist_to_obs < best) { best = dist_to_obs; bq = qj; }            // :569-575 (first strict minimum)
        }
        // block argmin with the sequential loop's tie rule (lowest obstacle index among equal distances)
        const double wmin = wave_min(best);
        if (lane == 0) S.red[0][0][wave] = wmin;
        if (tid == 0) S.itmp = 0x7fffffff;
        __syncthreads();
        if (checks && any_slack) S.gen = 1;       // (initialised by lane 0 in front of that barrier; every writer stores the same value; read behind the next one)
        double dmin = S.red[0][0][0];
#pragma unroll
        for (int w = 1; w < NWAVE; w++) dmin = fmin(dmin, S.red[0][0][w]);
        if (bq != 0x7fffffff && best == dmin) atomicMin(&S.itmp, bq);
        __syncthreads();
        if (tid == 0) {
            F3 g;
            if (dmin < a.priority_dist_threshold) g = rule_retreat_goal(pos, a.state + 9 * S.itmp, a.priority_dist_threshold);
            else {
                // initial_traj[M-1][n] (the current position when the initial trajectory was reset / in BVC mode)
                const float end[3] = {rest ? pos[0] : S.pinit[cl], rest ? pos[1] : S.pinit[SEGV + cl], rest ? pos[2] : S.pinit[2 * SEGV + cl]};
                g = rule_los_free_goal(goal_i, end, a.goal_radius);
            }
            S.goalf[0] = g.x; S.goalf[1] = g.y; S.goalf[2] = g.z;
        }
    } else if (tid < 3) {
        S.goalf[tid] = a.goal[3 * qi + tid];
    }
    // (roles: from here to barrier (1) nothing is left to do -- the goal, its terminal segments, the box bounds and the tables are the goal wave's
    //  and the copy waves' work of phase B)
    if (!roles) __syncthreads();
    if (tid < 3 && !roles) {
        const int k = tid;
        const float *s = a.state + 9 * qi;
        // planar world: z is not a variable (deq has two columns, src/traj_optimizer.cpp:239-259); the z unknowns of this solver
        // rest at z_2d -- state constants and terminal target there, no rows -- and are overwritten on output
        // (rule_state_constants, kept as inline text: as a call it costs lsc_plan_batch_kernel<true, true, 0> four bytes of scratch)
        double c0 = (double)s[k];
        double c1 = c0 + (double)s[3 + k] * md.hv_scale;
        double c2 = (double)s[6 + k] * md.ha_scale + 2.0 * c1 - c0;
        if (dim2 && k == 2) c0 = c1 = c2 = md.z2d;
        S.s0[k][0] = c0; S.s0[k][1] = c1; S.s0[k][2] = c2;
        if constexpr (TABLES_IN_LDS) { S.x0c[k * SEGV] = c0; S.x0c[k * SEGV + 1] = c1; S.x0c[k * SEGV + 2] = c2; }
        S.goal[k] = (dim2 && k == 2) ? md.z2d : (double)S.goalf[k];
        S.vlim[k] = a.vmax[3 * qi + k] * md.hv_scale; S.alim[k] = a.amax[3 * qi + k] * md.ha_scale;      // (every later phase reads these: no second trip to HBM)
        if (a.goal_out) a.goal_out[3 * qi + k] = S.goalf[k];
        for (int m = 0; m < M; m++) {
            double lo, hi;
            rule_box_bounds(md.world_min[k], md.world_max[k], a.sfc + ((size_t)qi * M + m) * 6, md.use_sfc && a.sfc, k, true, lo, hi);
            S.lo[k][m] = lo; S.hi[k][m] = hi;
        }
    }
    if (tid == 0 && !roles) S.tseg = rule_terminal_segments(S.goalf, a.state + 9 * qi, a.vnom[qi], md.dt);
    // per-lane solver constants -> LDS tables (see Smem)
    // lanes 0..89 (x / objective) and the last 90 (row gather) work on variable (xk, xt).  Computed twice -- here for the tables
    // of phase A and again behind phase B, from a copy of tid the compiler cannot see through -- so that the pair is not live
    // across the GJK pass, where it was the value that went to scratch (0.4 MB of scratch writes per launch in the PMC pass).
    int xk, xt;
    auto lane_variable = [&]() {
        int tq = tid;
        asm volatile("" : "+v"(tq));
        const int vq = tq < NV ? tq : (tq >= NT - NV ? tq - (NT - NV) : -1);
        xk = vq >= 0 ? vq / SEGV : 0;
        xt = vq >= 0 ? vq % SEGV : 0;
    };
    lane_variable();
    // Agent-independent tables.  SOLVER == 1: plain copies of the host's images (Model::amap32, xgp32, xtcm, Qh) -- every workgroup used to derive
    // them behind dependent loads of the model's fields.  (At the top of the kernel, with its first loads, the copies cost four spilled registers;
    // here none.)  The interior-point instantiations keep deriving them: with the copies THEY spilled a register.
    if (roles) {
        // (the copy waves' work, beside the GJK: role_tables below)
    } else if constexpr (SOLVER == 1) {
        for (int i = tid; i < n_ax; i += NT) S.amap[i] = md.amap32[i];
        for (int i = tid; i < NV; i += NT) S.xgp[i] = md.xgp32[i];
        for (int i = tid; i < SEGV * 3; i += NT) S.xtc[i / 3][i % 3] = md.xtcm[i / 3][i % 3];
        for (int i = tid; i < NC * NC; i += NT) S.Qh6[i] = md.Qh[i];
    } else {
        for (int i = tid; i < n_ax; i += NT) {
            const uint32_t sl = md.amap[i], type = sl / NV, kt = sl % NV;
            S.amap[i] = sl | (type << 10) | ((kt / SEGV) << 13) | ((kt % SEGV) << 15);
        }
        if (tid < NV) {
            const int xn = md.x_n[xt];
            S.xgp[tid] = (uint32_t)yglob(xk, md.x_i[xt][0]) | ((uint32_t)yglob(xk, md.x_i[xt][1]) << 8) |
                         ((uint32_t)yglob(xk, md.x_i[xt][2]) << 16);
            if (xk == 0) {
                S.xtc[xt][0] = xn < 1 ? 0.0 : md.x_c[xt][0];
                S.xtc[xt][1] = xn < 2 ? 0.0 : md.x_c[xt][1];
                S.xtc[xt][2] = xn < 3 ? 0.0 : md.x_c[xt][2];
            }
        } else if (tid >= 128 && tid < 128 + NC * NC) {
            S.Qh6[tid - 128] = md.Qh[tid - 128];
        }
    }
    // (what follows is the interior point's alone: with SOLVER == 1 it is built in ip_late_setup)
    auto ip_ytables = [&](const int t0 = 192) {
      if (tid >= t0 && tid < t0 + NY) {
        const int g = tid - t0;
        const int yk = yaxis(g);
        const int va = yvar(g);
        const int n = md.t_n[va];
        S.ytc[g][0] = n > 0 ? md.t_c[va][0] : 0.0; S.ytc[g][1] = n > 1 ? md.t_c[va][1] : 0.0;
        S.ytc[g][2] = n > 2 ? md.t_c[va][2] : 0.0; S.ytc[g][3] = n > 3 ? md.t_c[va][3] : 0.0;
        const int t0 = n > 0 ? md.t_t[va][0] : 0, t1 = n > 1 ? md.t_t[va][1] : 0;
        const int t2 = n > 2 ? md.t_t[va][2] : 0, t3 = n > 3 ? md.t_t[va][3] : 0;
        S.yop[g] = (uint32_t)(yk * SEGV + t0) | ((uint32_t)(yk * SEGV + t1) << 8) | ((uint32_t)(yk * SEGV + t2) << 16) |
                   ((uint32_t)(yk * SEGV + t3) << 24);
        S.ypp[g] = (uint32_t)(t0 * 3 + yk) | ((uint32_t)(t1 * 3 + yk) << 8) | ((uint32_t)(t2 * 3 + yk) << 16) |
                   ((uint32_t)(t3 * 3 + yk) << 24);
      }
    };
    if constexpr (SOLVER != 1) if (!roles) ip_ytables();
    __syncthreads();      // (roles: barrier (1))
    // constant part of every Hessian entry: cost Hessian (same axis) + terminal weight on c_{m,5}
    auto kconst_of = [&](uint32_t id) -> double {
        const int gi = id >> 16, gj = id & 0xffff;
        const int ki = yaxis(gi), kj = yaxis(gj);
        const int va = yvar(gi), vb = yvar(gj);
        double v = 0.0;
        if (ki == kj) {
            v = md.Hc[va * NYA + vb];
            if (va == vb) {
                const int mterm = va == NYL ? M - 1 : ((va % 3) == 2 ? va / 3 : -1);
                if (mterm >= M - S.tseg) v += 2.0 * md.w_t;
            }
        }
        return v;
    };
    // (roles: S.tseg is published by barrier (3); the constant parts are formed behind it)
    if constexpr (SOLVER != 1) for (int e = tid; e < (roles ? 0 : n_entries); e += NT) kconst[e] = kconst_of(ent[2 * e]);
    // Axis-row slot sl: whether the row exists and its right-hand side, stored to S.avalid / S.ah (and, for the interior point, the slot's
    // start values); returns the right-hand side.
    auto ax_slot = [&](const int sl) -> double {
        const AxisSlot s = axis_slot_of(sl);
        double h;
        const bool valid = rule_axis_row(s, dim2, S.hi[s.k][s.m], S.lo[s.k][s.m], S.vlim[s.k], S.alim[s.k], h);
        if constexpr (TABLES_IN_LDS) S.avalid[sl] = valid ? 1 : 0;
        if constexpr (TABLES_IN_LDS) S.ah[sl] = h;
        if constexpr (SOLVER != 1) { S.as_[sl] = 1.0; S.az[sl] = 0.0; S.at1[sl] = 0.0; S.at2[sl] = 0.0; }
        return h;
    };
    // Active-set solve (gi_solve below): the stride of a working-set row in y-space and the capacity of the working set, which lives in the idle S.K
    constexpr int GS = (NY + 1) & ~1;                         // (40 for NY = 39)
    constexpr int GQ = (12 * GS + 12 * 12 + 2 * 12 + 6 <= NY * KLD) ? 12 : 8;      // what fits the idle K (12 in the M = 5 and the M = 4 build)
    // x from y for the variables v0 and v1 of this lane (lane and lane + 64 of a wave), with what never changes during a solve -- the y-indices and
    // coefficients of the two variables, their state constants -- given by the caller from its registers: one batch of six loads of y per call.
    // The y values may have been written by other lanes of this wave just before: LDS operations of a wave complete in order, so a wave-level
    // fence stands for the workgroup barrier.
    auto gi_x_lanes = [&](const int xv0, const int xv1, const uint32_t xg0, const uint32_t xg1, const double xa00, const double xa01, const double xa02,
                          const double xa10, const double xa11, const double xa12, const bool xs0, const bool xs1, const double xk0, const double xk1) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double y00 = S.y[xg0 & 0xff], y01 = S.y[(xg0 >> 8) & 0xff], y02 = S.y[xg0 >> 16], y10 = S.y[xg1 & 0xff], y11 = S.y[(xg1 >> 8) & 0xff], y12 = S.y[xg1 >> 16];
        LSC_PIN(PV(y00), PV(y01), PV(y02), PV(y10), PV(y11), PV(y12));
        S.x[xv0] = xs0 ? xk0 : xa00 * y00 + xa01 * y01 + xa02 * y02;
        if (lane + 64 < NV) S.x[xv1] = xs1 ? xk1 : xa10 * y10 + xa11 * y11 + xa12 * y12;
    };
    constexpr int GW_NPRE = (SEGV * NYA + 63) / 64, CW_NPRE = (SEGV * NYA + COPY_NT - 1) / COPY_NT;      // gi_hz per lane of the goal wave, gi_zt per lane of the copy waves
    // The copy waves' work (roles): the agent-independent tables above, strided over their lanes.  Nothing reads them before barrier (3).
    // SOLVER == 1: and the start of the active-set solve as far as it hangs on nothing but barrier (1) and the model -- gi_zt, the velocity and
    // acceleration slots of S.ah / S.avalid with their selection scales, the zeros of the working set (the bound slots, gi_hz, y and x: goal wave).
    auto role_tables = [&]() {
        const int ct = tid - COPY_T0;
        if constexpr (SOLVER == 1) {
            double zt[CW_NPRE];
#pragma unroll
            for (int u = 0; u < CW_NPRE; u++) {
                const int i = ct + u * COPY_NT < SEGV * NYA ? ct + u * COPY_NT : 0;
                zt[u] = md.gzt[i];
            }
            for (int i = ct; i < n_ax; i += COPY_NT) S.amap[i] = md.amap32[i];
            for (int i = ct; i < NV; i += COPY_NT) S.xgp[i] = md.xgp32[i];
            for (int i = ct; i < SEGV * 3; i += COPY_NT) S.xtc[i / 3][i % 3] = md.xtcm[i / 3][i % 3];
            for (int i = ct; i < NC * NC; i += COPY_NT) S.Qh6[i] = md.Qh[i];
            for (int sl = 2 * NV + ct; sl < AXROWS; sl += COPY_NT) S.at2[sl] = rcp_nr(1.0 + fabs(ax_slot(sl)));
            for (int i = ct; i < GQ * GS + GQ * GQ + 2 * GQ; i += COPY_NT) S.K[i] = 0.0;      // Yw, Si, uw, rwv of gi_solve
#pragma unroll
            for (int u = 0; u < CW_NPRE; u++) if (ct + u * COPY_NT < SEGV * NYA) S.az[ct + u * COPY_NT] = zt[u];
        } else {
            static_assert(!SEG_WAVES || NY <= COPY_NT, "ip_ytables: one lane per free variable");
            for (int i = ct; i < n_ax; i += COPY_NT) {
                const uint32_t sl = md.amap[i], type = sl / NV, kt = sl % NV;
                S.amap[i] = sl | (type << 10) | ((kt / SEGV) << 13) | ((kt % SEGV) << 15);
            }
            for (int v = ct; v < NV; v += COPY_NT) {
                const int vk = v / SEGV, vt = v % SEGV, xn = md.x_n[vt];
                S.xgp[v] = (uint32_t)yglob(vk, md.x_i[vt][0]) | ((uint32_t)yglob(vk, md.x_i[vt][1]) << 8) |
                           ((uint32_t)yglob(vk, md.x_i[vt][2]) << 16);
                if (vk == 0) {
                    S.xtc[vt][0] = xn < 1 ? 0.0 : md.x_c[vt][0];
                    S.xtc[vt][1] = xn < 2 ? 0.0 : md.x_c[vt][1];
                    S.xtc[vt][2] = xn < 3 ? 0.0 : md.x_c[vt][2];
                }
            }
            for (int i = ct; i < NC * NC; i += COPY_NT) S.Qh6[i] = md.Qh[i];
            ip_ytables(COPY_T0);
        }
    };
    // Throughput build: the entry words of this lane's (at most two) Hessian entries never change -- kept in registers --, and the term
    // words they point at are fetched from L2 in ONE batch in front of every row reduction (prefetch_terms), so that the assembly
    // behind it finds them in registers: read where they were needed they cost up to three dependent L2 round trips per assembly.
    stamp(PH_SETUP);

    // SOLVER == 1: this solve's H^-1 block and its table H^-1 Z' e_t (Model::ginv, ghz) are fetched behind the GJK pass and its registers
    // (gi_prefetch, called in phase B) -- the values travel while the rows are bucketed and sorted -- and stored at the start of the active-set
    // solve (fetched there, the trip to L2 stood in front of the solve: ~0.7 us per agent-tick)
    constexpr int GI_NPRE = (SEGV * NYA + NTT - 1) / NTT;
    double gi_pre_z[GI_NPRE], gi_pre_n[GI_NPRE], gi_pre_y[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < GI_NPRE; u++) { gi_pre_z[u] = 0.0; gi_pre_n[u] = 0.0; }
    // (roles: not called -- the tables are fetched and stored by the goal wave and the copy waves beside the GJK)
    auto gi_prefetch = [&]() {
        if constexpr (SOLVER == 1) {
            const double *zsrc = md.ghz[S.tseg - 1], *ysrc = md.gy0[S.tseg - 1] + 4 * (tid < NY ? yvar(tid) : 0);
#pragma unroll
            for (int u = 0; u < GI_NPRE; u++) {
                const int i = tid + u * NTT < SEGV * NYA ? tid + u * NTT : 0;
                gi_pre_z[u] = zsrc[i];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) gi_pre_y[j] = ysrc[j];      // (the unconstrained optimum is linear in the state constants and the goal: Model::gy0)
#pragma unroll
            for (int u = 0; u < GI_NPRE; u++) {
                const int i = tid + u * NTT < SEGV * NYA ? tid + u * NTT : 0;
                gi_pre_n[u] = md.gzt[i];
            }
        }
    };
    // slot tables of the row reduction (interior point), in two halves around a barrier: offsets by one half-wave per table, then the entries
    auto slot_offsets = [&](int which, int b, int c, int total) {
        const int cap_slots = which == 0 ? RSLOT_P : RSLOT_C, min_rpl = 4;
        int rpl = (total + (cap_slots - NB) - 1) / (cap_slots - NB);
        rpl = rpl < min_rpl ? min_rpl : rpl;
        const int parts = b < NB ? (c + rpl - 1) / rpl : 0;
        int pin = parts;
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) {
            const int up = __shfl_up(pin, d, 32);
            if (b >= d) pin += up;
        }
        unsigned short *so = which == 0 ? S.soffP : S.soffC;
        if (b <= NB) so[b] = (unsigned short)(pin - parts);
        if (b == 0) S.rpl[which] = rpl;
    };
    auto slot_entries = [&]() {
        for (int q = tid; q < 2 * NB; q += NT) {
            const int which = q >= NB, b = which ? q - NB : q;
            const unsigned short *so = which ? S.soffC : S.soffP;
            uint32_t *sl = which ? S.slotC : S.slotP;
            const int rpl = S.rpl[which], cnt = S.cnt[b + 3], r0 = S.offs[b];
            for (int p = 0, s = so[b]; p * rpl < cnt; p++, s++) {
                const int n = cnt - p * rpl < rpl ? cnt - p * rpl : rpl;
                sl[s] = (uint32_t)(r0 + p * rpl) | ((uint32_t)n << 16) | ((uint32_t)b << 24);
            }
        }
    };
    // bucket offsets, and (rows in LDS) the slot tables of the row reduction -- bucket b is cut into parts of rpl rows; rpl is the smallest
    // that fits the staging --: one lane per bucket (and table), offsets by 32-lane prefix sums, run by a whole wave (both halves scan).  (One lane
    // walking the 27 buckets for the offsets and two walking them with a division each for the tables were ~900 instructions on a wave
    // everybody waited for.)  SEGW: the counts come from the segment waves (S.wcnt[0], see phase B) and S.cnt is written here; every segment
    // wave scans for itself (excl: the offset of this lane's bucket, over: more rows than R), only the publishing wave stores anything.
    static_assert(NB < 32, "one half-wave per bucket table");
    auto bucket_offsets = [&](const bool SEGW, const bool publish, int &excl, bool &over) {
        const int which = lane >> 5, b = lane & 31;
        int c = b < NB ? (SEGW ? S.wcnt[0][b + 3] : S.cnt[b + 3]) : 0;
        int incl = c, mx = c;
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) {
            const int up = __shfl_up(incl, d, 32);
            if (b >= d) incl += up;
            mx = max(mx, __shfl_xor(mx, d, 32));
        }
        int total = __shfl(incl, 31, 32);
        over = total > R;                            // more rows than this pass holds: left to the pass with the rows in HBM
        if (over) { c = 0; incl = 0; total = 0; }
        excl = incl - c;
        if (!publish) return;
        if (which == 0) {
            if (b < NB) { S.offs[b] = incl - c; S.offcnt[b] = (uint32_t)(incl - c) | ((uint32_t)c << 16); }
            if (SEGW) { if (b < NB) S.cnt[b + 3] = c; }      // (entries 0-2, the fixed control points, are zero since the top of the kernel)
            else if (over) S.cnt[b] = 0;
            if (b == 0) {
                if (a.bucket_max) a.bucket_max[qi] = mx;     // diagnostics: the fullest control-point bucket
                if (over) S.flag = 1;
                S.nact = total;
            }
        }
        if constexpr (!SPILL && SOLVER != 1) slot_offsets(which, b, c, total);
    };

    // ------------------------------------------------------------------ phase B: LSC rows
    // unit = (obstacle oi, segment m); rows that cannot be active inside the reachable box are dropped
    // (redundant constraints: removing them does not change the feasible set, hence not the optimum).
    {
        const double r_a = a.radius[qi], dw_a = a.downwash[qi];
        const double dlx = S.vlim[0], dly = S.vlim[1], dlz = S.vlim[2];   // largest step between consecutive control points (vmax dt / n)
        const int n_units = (ALT && S.gen) ? 0 : n_obs * M;    // alternate-mode QP: rows are built by lsc_general_kernel
        const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
        // Reachable box of every control point relative to c_{0,2}.  Consecutive control points differ by at most
        // V = vmax dt/n (velocity rows, traj_optimizer.cpp:472-492) and consecutive differences by at most
        // A = amax dt^2/(n(n-1)) (acceleration rows :494-523; C1/C2 continuity carries both across segment ends), and the
        // first difference d0 = c_{0,2} - c_{0,1} is fixed by the current state.  Hence after K steps, per axis,
        //   sum_{j<=K} max(-V, d0 - jA)  <=  c - c_{0,2}  <=  sum_{j<=K} min(V, d0 + jA).
        // (one lane per step and axis, the sums by a 32-lane prefix scan: three lanes walking the 27 steps were 1.2 us per tick on a wave
        //  everybody waited for.  The scan adds in another order than the walk -- a few ulp, against a 1e-9 pad per step.)
        if (tid < 96) {
            const int k = tid >> 5, j = tid & 31;
            const double V = S.vlim[k], A = S.alim[k];
            const double d0 = S.s0[k][2] - S.s0[k][1];
            const bool in = j >= 1 && j < 28;
            double lo = in ? fmax(-V, d0 - (double)j * A) - 1e-9 : 0.0;
            double hi = in ? fmin(V, d0 + (double)j * A) + 1e-9 : 0.0;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const double ul = __shfl_up(lo, d, 32), uh = __shfl_up(hi, d, 32);
                if (j >= d) { lo += ul; hi += uh; }
            }
            if (j < 28) { S.reachL[k][j] = lo; S.reachU[k][j] = hi; }
        }
        __syncthreads();      // (roles: barrier (2))
        // (the goal wave's work stands HERE, in front of the cull's code, and not in the chain of roles below: what it carries from its scan would
        //  otherwise be live across that code, whose registers are the scarce ones)
        if (goal_wave) {
            // ---- goal wave: between barriers (2) and (3) the rest of goal planning, every value the same in all its lanes (no barrier, no LDS
            // round trip inside the wave: the rules of the generic path's lone lanes, called by the whole wave on uniform values)
            const float *pos = a.state + 9 * qi;
            const float *goal_i = a.goal + 3 * qi;
            F3 g;
            if (a.goal_mode == 1) {
                // argmin with the sequential loop's tie rule (lowest obstacle index among equal distances): lane order is agent order within
                // a round, and a candidate of the first round (index below 64) goes in front of one of the second
                const double dmin = wave_min(gw_best);
                const unsigned long long tie = __ballot(gw_bq != 0x7fffffff && gw_best == dmin);
                const unsigned long long tie0 = __ballot(gw_bq < 64 && gw_best == dmin);
                const unsigned long long pick = tie0 != 0ull ? tie0 : tie;
                const int wl = __builtin_amdgcn_readfirstlane(pick != 0ull ? __ffsll((long long)pick) - 1 : 0);
                const int cl = (M - 1) * NC + DEG;                                    // control point [M-1][n]
                if (dmin < a.priority_dist_threshold) {
                    // the partner's position: the float32 values the lane that holds it fetched for the scan (no second trip to memory)
                    const float opos[3] = {__int_as_float(__builtin_amdgcn_readlane(__float_as_int(gw_opos[0]), wl)),
                                           __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gw_opos[1]), wl)),
                                           __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gw_opos[2]), wl))};
                    g = rule_retreat_goal(pos, opos, a.priority_dist_threshold);
                } else {
                    // initial_traj[M-1][n] (the current position when the initial trajectory was reset / in BVC mode)
                    const float end[3] = {rest ? pos[0] : S.pinit[cl], rest ? pos[1] : S.pinit[SEGV + cl], rest ? pos[2] : S.pinit[2 * SEGV + cl]};
                    g = rule_los_free_goal(goal_i, end, a.goal_radius);
                }
            } else g = F3{goal_i[0], goal_i[1], goal_i[2]};                          // static: current goal = the goal input
            if (lane < 3) {
                const int k = lane;
                const float gk = k == 0 ? g.x : (k == 1 ? g.y : g.z);
                S.goalf[k] = gk;
                S.goal[k] = (dim2 && k == 2) ? md.z2d : (double)gk;
                if (a.goal_out) a.goal_out[3 * qi + k] = gk;
                for (int m = 0; m < M; m++) {
                    double lo, hi;
                    rule_box_bounds(md.world_min[k], md.world_max[k], a.sfc + ((size_t)qi * M + m) * 6, md.use_sfc && a.sfc, k, true, lo, hi);
                    S.lo[k][m] = lo; S.hi[k][m] = hi;
                }
            }
            // (SOLVER == 1: formed by every lane from values that are the same in all of them -- the early start below picks its tables by it)
            if (SOLVER == 1 || lane == 0) {
                const float g3[3] = {g.x, g.y, g.z};
                gw_T = rule_terminal_segments(g3, pos, gw_vnom, md.dt);
                if (lane == 0) S.tseg = gw_T;
            }
        }
        // ---- goal wave, SOLVER == 1: the start of the active-set solve as far as it hangs on the goal -- gi_hz and the unconstrained optimum
        // (both picked by T), the bound slots of S.ah / S.avalid with their selection scales, x from y -- while the segment waves run the GJK.
        // A block of its own: these statements come from behind barrier (4) and are compiled as there, with the default contraction.
        if constexpr (SOLVER == 1) if (goal_wave) {
            const int T = __builtin_amdgcn_readfirstlane(gw_T);      // (the same in all lanes, and SAID to be: it picks the tables)
            const double *zsrc = md.ghz[T - 1], *ysrc = md.gy0[T - 1] + 4 * (lane < NY ? yvar(lane) : 0);
            double hz[GW_NPRE], y4[4];
#pragma unroll
            for (int u = 0; u < GW_NPRE; u++) {
                const int i = lane + u * 64 < SEGV * NYA ? lane + u * 64 : 0;
                hz[u] = zsrc[i];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) y4[j] = ysrc[j];      // (the unconstrained optimum is linear in the state constants and the goal: Model::gy0)
            // x from y by the host's images themselves: what the copy waves copy to S.xgp / S.xtc, and no barrier lies between the two roles
            const int xv0 = lane, xv1 = lane + 64 < NV ? lane + 64 : lane;
            const uint32_t xg0 = md.xgp32[xv0], xg1 = md.xgp32[xv1];
            const double xa00 = md.xtcm[xv0 % SEGV][0], xa01 = md.xtcm[xv0 % SEGV][1], xa02 = md.xtcm[xv0 % SEGV][2];
            const double xa10 = md.xtcm[xv1 % SEGV][0], xa11 = md.xtcm[xv1 % SEGV][1], xa12 = md.xtcm[xv1 % SEGV][2];
            const bool xs0 = xv0 % SEGV < 3, xs1 = xv1 % SEGV < 3;
            const double xk0 = xs0 ? S.x0c[xv0] : 0.0, xk1 = xs1 ? S.x0c[xv1] : 0.0;
            // S.goal, S.lo, S.hi: written by lanes 0 .. 2 above, read by every lane below
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int sl = lane; sl < 2 * NV; sl += 64) S.at2[sl] = rcp_nr(1.0 + fabs(ax_slot(sl)));
#pragma unroll
            for (int u = 0; u < GW_NPRE; u++) if (lane + u * 64 < SEGV * NYA) S.as_[lane + u * 64] = hz[u];
            if (lane < 40) {
                const int k = lane < NY ? yaxis(lane) : 0;
                double yv = y4[0] * S.s0[k][0] + y4[1] * S.s0[k][1] + y4[2] * S.s0[k][2] + y4[3] * S.goal[k];
                if (dim2 && k == 2) yv = md.z2d;          // planar world: y_z rests at z_2d (see gi_solve)
                S.y[lane] = lane < NY ? yv : 0.0;
            }
            gi_x_lanes(xv0, xv1, xg0, xg1, xa00, xa01, xa02, xa10, xa11, xa12, xs0, xs1, xk0, xk1);
        }
        // ---- spatial pre-cull (large swarms): most obstacles are so far away that every row against them is redundant,
        // and that can be seen without the GJK.  With w_j = p~_j - q~_j (scaled space), centroid w_c, R_w = max |w_j - w_c|:
        // the closest point v of conv{w_j} to the origin has |v| >= |w_c| - R_w and n~.w >= |v| on the hull (n~ = v/|v|).  A row
        // asks  n~.(c~ - p~_i) + (1/2) n~.(p~_i - q~_i) >= (1/2)(r_a + r_o); every reachable c lies within rho_K of c_{0,2}, so
        //   (1/2)(|w_c| - R_w) - s (|c_{0,2} - p_i| + rho_K) >= (1/2)(r_a + r_o) + margin,   s = max(1, 1/downwash)
        // implies the exact per-row test below (whose box is inside that sphere) for all rows of the unit: the unit is
        // dropped before the GJK and the surviving units -- the same rows in the same order as without the cull, hence
        // bit-identical plans -- are compacted so that whole waves do not idle behind a few near obstacles.
        const int prune_mode = md.prune == 3 ? 1 : md.prune;      // 3: exact test only (parity tests of the cull itself)
        // The unit list lives in rn .. cmap (16 B per row, contiguous, first written by the scatter that ends phase B).  (Until round 6 it started
        // at rrhs with a capacity of 12 R entries "in rrhs, rn and cmap" -- but indexed linearly, so that entries beyond 4 R lay in rs .. rt2,
        // where the GJK passes put their temporary rows: a swarm crowded enough for more than 4 R surviving units per agent -- 1024 agents in
        // 14 x 14 x 9 m, found by tests/fuzz_neighbours.py -- read overwritten entries and faulted.)
        uint16_t *ulist = reinterpret_cast<uint16_t *>(rn);
        const int list_cap = 8 * R;
        // Entries are the low 16 bits of the unit.  Above 13 107 agents (M = 5) a unit needs up to 19 bits: the list stays ascending, so the
        // high part of entry i is the number of k with i >= ublk[k], ublk[k] = first entry whose unit is >= (k + 1) << 16 (0x7fffffff: none).
        // The four words are S.offs[0..3]: the bucket offsets are first written behind the GJK pass, and a 16-bit entry keeps the capacity.
        int *const ublk = S.offs;
        const bool wide = n_units > 0xffff;
        // Large swarms: the units worth looking at come as a list from lsc_neigh.hip (built through a uniform grid in front of the tick: a
        // superset of what the cull below keeps, in the same ascending order -- the exact per-row test decides in both cases, so the rows
        // are the same); an agent without a list (capacity overflow there) culls by itself.
        const NeighView *const nvb = a.nv;
        const int n_given = (nvb != nullptr && md.prune == 1 && !a.out_normal && n_units > 0) ? __builtin_amdgcn_readfirstlane(nvb->cnt[qi]) : -1;
        const bool given = n_given >= 0 && n_given <= list_cap;
        bool cull = md.prune == 1 && !a.out_normal && n_units > NT && n_units <= NEIGH_MAX_UNITS;
        int n_list = n_units;
        if (given) {
            // the list moves into the LDS slots of the in-kernel cull's own list: the GJK pass below reads it there (read from HBM inside the
            // pass, the address and the entry cost the production kernels the registers that keep them free of scratch)
            const unsigned short *glist = uniform_ptr(nvb->list) + (size_t)qi * __builtin_amdgcn_readfirstlane(nvb->cap);
            for (int i = tid; i < n_given; i += NT) ulist[i] = glist[i];
            if (tid < 4) {
                // (lsc_neigh.hip: four 16-bit starts per agent, 0xffff = none; a list within list_cap < 0xffff never reaches one)
                const unsigned s = wide ? (unsigned)(uniform_ptr(nvb->blk)[qi] >> (16 * tid)) & 0xffffu : 0xffffu;
                ublk[tid] = s == 0xffffu ? 0x7fffffff : (int)s;
            }
            cull = true;
            n_list = n_given;
            __syncthreads();
        } else if (cull) {
            if (tid == 0) S.listfull = 0;
            if (tid < 4) ublk[tid] = 0x7fffffff;
            // Reach of every control point (distance from c_{0,2} + radius of its reachable box), per segment (cullB) and overall (cullA), one
            // lane of wave 0 per control point.  (Five lanes walking six points each, then one lane walking all thirty, were ~450 instructions on
            // lone lanes and a barrier of their own: ~1.5 us per agent-tick of a large swarm.)
            if (wave == 0) {
                const int c = lane < SEGV ? lane : SEGV - 1, K = 5 * (c / NC) + (c % NC) - 2;
                const int Kc = K >= 1 ? K : 1;
                double d2 = 0.0, r2 = 0.0;
                for (int k = 0; k < 3; k++) {
                    const double dd = S.s0[k][2] - (double)S.pinit[k * SEGV + c];
                    const double e = fmax(fabs(S.reachL[k][Kc]), fabs(S.reachU[k][Kc]));
                    d2 += dd * dd; r2 += e * e;
                }
                const double bc = (lane < SEGV && K >= 1) ? sqrt(d2) + sqrt(r2) : 0.0;
                const double ra2 = wave_max(lane < SEGV ? d2 : 0.0), bm = wave_max(bc);
                double *const ct = reinterpret_cast<double *>(&S.colbuf[0][0]);      // (the factorisation's buffers are idle in phase B)
                if (lane < SEGV) ct[lane] = bc;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (lane < M) {
                    double bb = 0.0;
                    for (int i = 0; i < NC; i++) bb = fmax(bb, ct[lane * NC + i]);
                    S.cullB[lane] = bb;
                }
                if (lane == 0) { S.cullA[0] = sqrt(ra2); S.cullA[1] = bm; }
            }
            __syncthreads();
            // Obstacle level first (throughput build: lsc_prep_kernel left a bounding sphere (B_o, rho_o) of every agent's
            // predicted control points): all w_j of all segments lie in the ball around D = c_{0,2} - B_o (scaled space) of
            // radius s (rho_a + rho_o), so |w_c| >= |D| - s (rho_a + rho_o) and R_w <= 2 s (rho_a + rho_o); hence
            //   |D| >= s (3 (rho_a + rho_o) + 2 max_m B_m) + (r_a + r_o) + margin
            // implies the per-segment test below for all five segments.  Survivors keep their order, so the unit list --
            // and with it every plan -- is the same as without this level.
            uint16_t *olist = reinterpret_cast<uint16_t *>(rs);      // the (rs .. rt2) slots are first written by the GJK pass
            const bool lvl0 = !OBS && a.obs_bound != nullptr && n_obs <= (SPILL ? 0x7fffffff : 16 * R);      // (the bounds are the agents' alone)
            int n_o = n_obs;
            if (lvl0) {
                int tot0 = 0;
                for (int base = 0; base < n_obs; base += NT) {
                    const int oi = base + tid;
                    bool keep = false;
                    if (oi < n_obs) {
                        const int qj = oi < qi ? oi : oi + 1;
                        const float4 bo = reinterpret_cast<const float4 *>(a.obs_bound)[qj];
                        const double r_o = a.radius_obs[qj];
                        const double downwash = (dw_a * r_a + a.downwash_obs[qj] * r_o) / (r_a + r_o);
                        const double idw = 1.0 / downwash, sc = fmax(1.0, idw);
                        const double dx = S.s0[0][2] - (double)bo.x, dy = S.s0[1][2] - (double)bo.y, dz = (S.s0[2][2] - (double)bo.z) * idw;
                        const double need = sc * (3.0 * (S.cullA[0] + (double)bo.w) + 2.0 * S.cullA[1]) + (r_o + r_a) + 2e-4 + 1e-6;
                        keep = !(dx * dx + dy * dy + dz * dz >= need * need);
                    }
                    const unsigned long long mask = __ballot(keep);
                    if (lane == 0) S.cullc[wave] = __popcll(mask);
                    __syncthreads();
                    int cw[NWAVE];                     // (all counts in one batch of loads, not one LDS round trip per wave in front)
#pragma unroll
                    for (int w = 0; w < NWAVE; w++) cw[w] = S.cullc[w];
                    int off = tot0;
#pragma unroll
                    for (int w = 0; w < NWAVE; w++) { off += w < wave ? cw[w] : 0; tot0 += cw[w]; }
                    if (keep) olist[off + __popcll(mask & lt_mask)] = (uint16_t)oi;
                    __syncthreads();
                }
                n_o = tot0;
            }
            const int n_units1 = n_o * M;
            int total = 0;
            for (int base = 0; base < n_units1; base += NT) {
                const int u1 = base + tid;
                bool keep = false;
                const int oi = u1 < n_units1 ? (lvl0 ? (int)olist[u1 / M] : u1 / M) : 0, m = u1 % M;
                const int u = oi * M + m;
                if (u1 < n_units1) {
                    const int qj = oi < qi ? oi : oi + 1;
                    F3 po[6];
                    const bool dyn = OBS && qj >= N;
                    if (dyn) rule_obstacle_segment(ob->pos_vel + 6 * (qj - N), m, dtf, po);
                    else load_segment(a.state, a.traj_prev, qj, m, a.planner_seq, dtf, po);
                    const double r_o = dyn ? ob->radius[qj - N] : a.radius_obs[qj];
                    const double downwash = dyn ? rule_pair_downwash(r_a, dw_a, r_o, ob->downwash[qj - N], false) : (dw_a * r_a + a.downwash_obs[qj] * r_o) / (r_a + r_o);
                    const double idw = 1.0 / downwash, sc = fmax(1.0, idw);
                    double wx[6], wy[6], wz[6], cx = 0.0, cy = 0.0, cz = 0.0;
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        const int c = m * NC + i;
                        wx[i] = (double)S.pinit[c] - (double)po[i].x;
                        wy[i] = (double)S.pinit[SEGV + c] - (double)po[i].y;
                        wz[i] = ((double)S.pinit[2 * SEGV + c] - (double)po[i].z) * idw;
                        cx += wx[i]; cy += wy[i]; cz += wz[i];
                    }
                    cx *= (1.0 / 6.0); cy *= (1.0 / 6.0); cz *= (1.0 / 6.0);
                    double rw2 = 0.0;
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        const double ex = wx[i] - cx, ey = wy[i] - cy, ez = wz[i] - cz;
                        rw2 = fmax(rw2, ex * ex + ey * ey + ez * ez);
                    }
                    const double need = 2.0 * sc * S.cullB[m] + (r_o + r_a) + 2e-4 + sqrt(rw2);
                    keep = !(cx * cx + cy * cy + cz * cz >= need * need);
                }
                const unsigned long long mask = __ballot(keep);
                if (lane == 0) S.cullc[wave] = __popcll(mask);
                __syncthreads();
                int cw[NWAVE];
#pragma unroll
                for (int w = 0; w < NWAVE; w++) cw[w] = S.cullc[w];
                int off = total;
#pragma unroll
                for (int w = 0; w < NWAVE; w++) { off += w < wave ? cw[w] : 0; total += cw[w]; }
                if (keep) {
                    const int at = off + __popcll(mask & lt_mask);
                    if (at < list_cap) ulist[at] = (uint16_t)u;
                    else S.listfull = 1;
                    if (wide)
                        for (int k = 0; k < (u >> 16); k++) atomicMin(&ublk[k], at);
                }
                __syncthreads();
            }
            if (S.listfull) cull = false;          // more survivors than the list holds: every unit takes the GJK
            else n_list = total;
        }
        // rows of unit (obstacle oi = agent qj, segment m): GJK, right-hand sides, which of the six survive the pruning
        auto unit_rows = [&](const int oi, const int m, const int qj, F3 &nrm, double (&rhs)[6], bool (&actv)[6]) {
            F3 pa[6], po[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                int c = m * NC + i;
                pa[i] = F3{S.pinit[c], S.pinit[SEGV + c], S.pinit[2 * SEGV + c]};
            }
            // (fetching the first round's segments ahead -- at the top of the kernel, or in front of the reach boxes' barrier -- was tried: the
            //  22 registers held across phase A / the cull code went to scratch, 64-96 B per lane on every instantiation)
            // (OBS: qj >= N is dynamic obstacle qj - N -- constant velocity at every planner_seq, the non-agent downwash rule)
            const bool dyn = OBS && qj >= N;
            if (dyn) rule_obstacle_segment(ob->pos_vel + 6 * (qj - N), m, dtf, po);
            else load_segment(a.state, a.traj_prev, qj, m, a.planner_seq, dtf, po);
            const double r_o = dyn ? ob->radius[qj - N] : a.radius_obs[qj];
            const double downwash = dyn ? rule_pair_downwash(r_a, dw_a, r_o, ob->downwash[qj - N], false) : (dw_a * r_a + a.downwash_obs[qj] * r_o) / (r_a + r_o);
            double d[6];
            lsc_segment(pa, po, downwash, r_o + r_a, nrm, d);
            if (a.out_normal) {
                size_t o = ((size_t)al * n_obs + oi) * M + m;
                a.out_normal[o * 3] = nrm.x; a.out_normal[o * 3 + 1] = nrm.y; a.out_normal[o * 3 + 2] = nrm.z;
#pragma unroll
                for (int i = 0; i < 6; i++) a.out_d[o * 6 + i] = d[i];
            }
            // planar world: the row is n_x (x - q_x) + n_y (y - q_y) - d >= 0, its z term exists only `if (dim == 3)`
            // (src/traj_optimizer.cpp:446-453); the dump above keeps the normal CollisionConstraints holds
            if (dim2) nrm.z = 0.0f;
            const double nx = (double)nrm.x, ny = (double)nrm.y, nz = (double)nrm.z;
            const double centre = nx * S.s0[0][2] + ny * S.s0[1][2] + nz * S.s0[2][2];
            const double (*rx)[28] = nx >= 0.0 ? S.reachL : S.reachU, (*ry)[28] = ny >= 0.0 ? S.reachL : S.reachU,
                         (*rz)[28] = nz >= 0.0 ? S.reachL : S.reachU;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double r = d[i];
                r += nx * (double)po[i].x;
                r += ny * (double)po[i].y;
                r += nz * (double)po[i].z;
                rhs[i] = r;
                bool on = !(m == 0 && i < 3);
                if (on && prune_mode) {
                    // smallest n.c over the reachable box of c_{m,i} (K = 5m+i-2 steps from c_{0,2})
                    const int K = 5 * m + i - 2;
                    double worst = centre + nx * rx[0][K] + ny * ry[1][K] + nz * rz[2][K];
                    if (prune_mode == 2) worst = centre - (double)K * (fabs(nx) * dlx + fabs(ny) * dly + fabs(nz) * dlz);   // velocity rows only
                    if (worst >= r + 1e-6) on = false;
                }
                actv[i] = on;
            }
        };
        // ---- small swarms: at most 64 obstacles, no cull, no list -- one pass of the loop below, in which every wave holds units of all M
        // segments, so that every control-point bucket receives rows from every wave: M x 6 predicated ballots per wave, a count matrix, a
        // cross-wave prefix pass between two barriers, rows staged in arrival order and scattered a barrier later.  Here instead wave w
        // carries segment m = w, lane = obstacle (M waves of N - 1 lanes: the same M wave-passes of GJK).  Bucket cp = 6 m + i then belongs to
        // ONE wave: a row's place in it is the number of lower lanes with that row (ascending obstacle, the order of the loop below), the
        // bucket's size one popcount.  One barrier publishes the counts, every segment wave scans the 27 of them for itself and stores its
        // rows from the registers they sit in straight to their final slots.  Same layout to the last bit: rn, rrhs, cmap, offs, offcnt,
        // cnt, nact (tests/test_gpu_small_swarm_build.py; LSC_GENERIC_LSC_BUILD keeps a context on the loop below).
        // What a segment wave holds across the barrier that publishes the counts, packed: which of the six rows exist as a bit mask, their
        // places in their buckets (below 64) as six bytes.
        int sw_m = 0;
        uint32_t sw_act = 0u, sw_rank[2] = {0u, 0u};
        bool sw_seg = false;
        F3 sw_nrm = F3{0.f, 0.f, 0.f};
        double sw_rhs[6];
#pragma unroll
        for (int i = 0; i < 6; i++) sw_rhs[i] = 0.0;
        // (`placed` was decided at the top of the kernel -- uniform, and SAID to be: behind a branch the compiler takes for divergent, what the
        //  segment waves hold would stay live -- and go to scratch -- across the generic pass.  The roles are an if / else chain for the same reason.)
        if (SEG_WAVES && placed) {
            sw_m = role_wave;
            sw_seg = sw_m < M;
            if (sw_seg) {
                // ---- segment wave: between barriers (2) and (3) the GJK of its segment
                const int oi = lane;
                const bool live = oi * M < n_units;               // (n_units = 0: the rows are built by the general solver)
                const int qj = oi < qi ? oi : oi + 1;
                bool actv[6];
#pragma unroll
                for (int i = 0; i < 6; i++) actv[i] = false;
                if (live) unit_rows(oi, sw_m, qj, sw_nrm, sw_rhs, actv);
                int mine = 0;
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    const unsigned long long mask = __ballot(actv[i]);
                    sw_act |= actv[i] ? 1u << i : 0u;
                    sw_rank[i / 3] |= (uint32_t)__popcll(mask & lt_mask) << (8 * (i % 3));
                    if (lane == i) mine = __popcll(mask);
                }
                if (lane < NC) S.wcnt[0][sw_m * NC + lane] = mine;
            } else if (sw_m != NWAVE - 1) {
                // ---- copy waves: between barriers (2) and (3) the solver's agent-independent tables
                role_tables();
            }
        } else for (int base = 0; base < n_list; base += NT) {
            const int pos_u = base + tid;
            const bool live = pos_u < n_list;
            int u = live ? (cull ? (int)ulist[pos_u] : pos_u) : 0;
            if (wide && cull) {
                u |= ((pos_u >= ublk[0]) + (pos_u >= ublk[1]) + (pos_u >= ublk[2]) + (pos_u >= ublk[3])) << 16;
            }
            const int oi = live ? u / M : 0, m = live ? u % M : 0;
            const int qj = oi < qi ? oi : oi + 1;
            F3 nrm = F3{0.f, 0.f, 0.f};
            double rhs[6];
            bool actv[6];
#pragma unroll
            for (int i = 0; i < 6; i++) { rhs[i] = 0.0; actv[i] = false; }
            if (live) unit_rows(oi, m, qj, nrm, rhs, actv);
            // deterministic bucketing by control point: rows of a bucket stay in increasing-obstacle order
            int rank[6];
#pragma unroll
            for (int i = 0; i < 6; i++) rank[i] = 0;
#pragma unroll
            for (int mm = 0; mm < M; mm++) {
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    unsigned long long mask = __ballot(live && m == mm && actv[i]);
                    if (m == mm) rank[i] = __popcll(mask & lt_mask);
                    if (lane == 0) S.wcnt[wave][mm * NC + i] = __popcll(mask);
                }
            }
            // arrival slots: one reservation per wave (the order is irrelevant, (cp, pos) decides the final place)
            int kslot = 0;
            {
                int pre = 0, tot = 0;
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    const unsigned long long mk = __ballot(live && actv[i]);
                    pre += __popcll(mk & lt_mask);
                    tot += __popcll(mk);
                }
                int base = 0;
                if (lane == 0 && tot) base = atomicAdd(&S.ntmp, tot);
                kslot = __builtin_amdgcn_readfirstlane(base) + pre;
            }
            __syncthreads();
            // first position of every wave's rows in every bucket: the bucket's count so far + the rows of the waves in front.  One lane per
            // (wave, control point), its loads in one batch; every row then needs ONE word.  (Each row used to walk the counts of the waves in
            // front of it, an LDS round trip per wave: up to 42 dependent trips per lane, 5 us per tick at 64 agents -- more than the GJK.)
            int *const wpre = reinterpret_cast<int *>(&S.colbuf[0][0]);      // [NWAVE + 1][32]; the factorisation's buffers are idle in phase B
            static_assert(sizeof(S.colbuf) >= sizeof(int) * (NWAVE + 1) * 32, "scratch of the bucket positions");
            if (tid < NWAVE * 32) {
                const int w = tid >> 5, cp = tid & 31;
                int c[NWAVE];
#pragma unroll
                for (int v = 0; v < NWAVE; v++) c[v] = S.wcnt[v][cp];
                int sum = S.cnt[cp];
#pragma unroll
                for (int v = 0; v < NWAVE; v++) sum += v < w ? c[v] : 0;
                wpre[w * 32 + cp] = sum;
                if (w == NWAVE - 1) wpre[NWAVE * 32 + cp] = sum + c[NWAVE - 1];      // the bucket's new count
            }
            __syncthreads();
            if (live) {
                int base[6];
#pragma unroll
                for (int i = 0; i < 6; i++) base[i] = wpre[wave * 32 + m * NC + i];
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    if (!actv[i]) continue;
                    const int cp = m * NC + i;
                    const int pos = base[i] + rank[i];      // position inside the bucket: obstacle order, deterministic
                    const int k = kslot++;
                    if (k < R) tmp_rows[k] = TmpRow{rhs[i], nrm.x, nrm.y, nrm.z, (uint32_t)cp | ((uint32_t)pos << 8)};
                }
            }
            if (tid < NCP) S.cnt[tid] = wpre[NWAVE * 32 + tid];      // (next read behind the next barrier: the next pass's, or the one below)
        }
        // this solve's tables are requested HERE: the GJK and its registers are behind, the values travel while the rows are placed
        if (!(SEG_WAVES && placed)) gi_prefetch();
        __syncthreads();      // (roles: barrier (3) -- publishes the segment waves' counts AND everything the goal wave and the copy waves wrote)
        {
            if (SEG_WAVES && placed && sw_seg) {
                int excl;
                bool over;
                bucket_offsets(true, sw_m == 0, excl, over);
                // (over: the agent is left to the pass with its rows in HBM and NO row is stored -- the slots beyond R are not this agent's)
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    const int cp = sw_m * NC + i;
                    const int r = __builtin_amdgcn_readlane(excl, cp >= 3 ? cp - 3 : 0) + (int)((sw_rank[i / 3] >> (8 * (i % 3))) & 0xffu);
                    if (((sw_act >> i) & 1u) != 0u && !over) {
                        rn[r] = sw_nrm.x; rn[R + r] = sw_nrm.y; rn[2 * R + r] = sw_nrm.z;
                        rrhs[r] = sw_rhs[i];
                        cmap[r] = (uint32_t)r | ((uint32_t)cp << CMAP_SHIFT);
                    }
                }
            }
        }
    }
    if (!placed && tid < 64) {
        int excl;
        bool over;
        bucket_offsets(false, true, excl, over);
    }
    __syncthreads();      // (roles: barrier (4))
    // (roles: the constant parts of the Hessian entries, which read S.tseg -- behind the rows' registers; the interior point reads them two barriers on)
    if constexpr (SOLVER != 1) for (int e = tid; e < (roles ? n_entries : 0); e += NT) kconst[e] = kconst_of(ent[2 * e]);
    if constexpr (!SPILL && SOLVER != 1) slot_entries();
    // scatter from arrival order to the compact, bucket-sorted layout
    for (int k = tid; k < (placed ? 0 : S.nact); k += NT) {
        const TmpRow t = tmp_rows[k];
        const int cp = (int)(t.cp_pos & 0xffu), pos = (int)(t.cp_pos >> 8);
        const int r = S.offs[cp - 3] + pos;
        rn[r] = t.nx; rn[R + r] = t.ny; rn[2 * R + r] = t.nz;
        rrhs[r] = t.rhs;
        cmap[r] = (uint32_t)r | ((uint32_t)cp << CMAP_SHIFT);
    }
    // (rows placed in phase B were stored in front of the barrier above; what follows up to the next barrier only writes tables of its own)
    if (!(placed && SOLVER == 1)) __syncthreads();
    stamp(PH_LSC);
    lane_variable();
    const bool xterm = (tid < NV) && (xt % NC == DEG) && (xt / NC >= M - S.tseg);

    // ------------------------------------------------------------------ phase C: interior point
    // Small swarms, SOLVER == 1: the start of the active-set solve -- the axis slots, the tables, the scales of the axis rows, the zeros of the
    // working set, the unconstrained optimum and its x -- was written by the goal wave and the copy waves in front of barrier (3); what is left
    // behind barrier (4) are the scales of this lane's own LSC rows and the registers of the first search: no barrier up to that search.
    // (`roles` is uniform and SAID to be, see `placed`)
    const bool early = SOLVER == 1 && roles;
    if (!early) for (int sl = tid; sl < AXROWS; sl += NT) ax_slot(sl);
    // right-hand side of axis row sl
    auto AH = [&](int sl) -> double {
        if constexpr (TABLES_IN_LDS) return S.ah[sl];
        else {
            const int type = sl / NV, kt = sl % NV, k = kt / SEGV, m = (kt % SEGV) / NC;
            return type == 0 ? S.hi[k][m] : (type == 1 ? -S.lo[k][m] : (type < 4 ? S.vlim[k] : S.alim[k]));
        }
    };
    if constexpr (SOLVER != 1) {
        if (tid < 40) { S.y[tid] = 0.0; S.dy[tid] = 0.0; }
        for (int i = tid; i < NY * KLD; i += NT) S.K[i] = 0.0;
        for (int i = tid; i < NCP * 3; i += NT) { S.Tv[i] = 0.0; S.Tz[i] = 0.0; }
        for (int i = tid; i < W_SIZE; i += NT) S.W[i] = 0.0;
    }
    if (!early) __syncthreads();
    const bool overflow = S.flag != 0;
    const int nact = S.nact;
    const double nrow = (double)(n_ax + nact);

    // state constant of variable v = k*SEGV + t (t < 3); existence of axis-row slot sl (the throughput build keeps neither table)
    auto X0C = [&](int v) -> double {
        if constexpr (TABLES_IN_LDS) return S.x0c[v];
        else return S.s0[v / SEGV][v % SEGV];
    };
    auto AVALID = [&](int sl) -> double {
        if constexpr (TABLES_IN_LDS) return (double)S.avalid[sl];
        else {
            const int type = sl / NV, kt = sl % NV, k = kt / SEGV, t = kt % SEGV, i = t % NC;
            const bool valid = type < 2 ? t >= 3 : (type < 4 ? (i <= 4 && t >= 2) : (i <= 3 && t >= 1));
            return (valid && !(dim2 && k == 2)) ? 1.0 : 0.0;
        }
    };
    // x from y : x_t = sum coef * y_glob  (+ state constants for t < 3)
    auto compute_x = [&](const double *yv, double *xv, bool with_const) {
        if (tid < NV) {
            double v;
            if (xt < 3) v = with_const ? X0C(tid) : 0.0;
            else {
                const uint32_t gp = S.xgp[tid];
                const double *c = S.xtc[xt];
                v = c[0] * yv[gp & 0xff] + c[1] * yv[(gp >> 8) & 0xff] + c[2] * yv[gp >> 16];
            }
            xv[tid] = v;
        }
    };
    // the same for ONE variable v, and for all variables on wave 0 alone (lane l: v = l and l + 64).  Used right behind a value
    // that wave 0 has just written itself (dy after the substitutions, y after the step): LDS operations of a wave complete in
    // order, so a wave-level fence replaces the workgroup barrier that used to sit between the two.
    auto x_of = [&](const double *yv, double *xv, bool with_const, int v) {
        const int t = v % SEGV;
        double val;
        if (t < 3) val = with_const ? X0C(v) : 0.0;
        else {
            const uint32_t gp = S.xgp[v];
            const double *c = S.xtc[t];
            val = c[0] * yv[gp & 0xff] + c[1] * yv[(gp >> 8) & 0xff] + c[2] * yv[gp >> 16];
        }
        xv[v] = val;
    };
    auto compute_x_wave0 = [&](const double *yv, double *xv, bool with_const) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        x_of(yv, xv, with_const, lane);
        if (lane + 64 < NV) x_of(yv, xv, with_const, lane + 64);
    };
    // cost gradient in x-space for this lane's variable: 2 w_c Q x within the segment (terminal term added by caller)
    auto cost_grad = [&]() -> double {
        const double *xs = S.x + xk * SEGV + (xt / NC) * NC;
        double g = 0.0;
#pragma unroll
        for (int j = 0; j < NC; j++) g += S.Qh6[(xt % NC) * NC + j] * xs[j];
        return g;
    };
    // block reduction of up to 5 values: op 0 sum, 1 max, 2 min; results in rv[0..4] (uniform registers).  One barrier: lane 0 of
    // every wave publishes the wave's partials, then EVERY wave combines them itself -- lane k walks slot k in wave order (the
    // summation order of rounds 1-3, so the results are the same bits) and the five results travel by v_readlane.  Round 3 had five
    // lanes of the workgroup combine, write S.sc and a second barrier in front of the read.  Two banks of partials, used in turn:
    // the next reduction may publish while a slow wave still reads this one's.
    // (op < 0: slot unused -- its wave reduction, ~45 instructions on every wave, is not emitted)
    double rv[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int red_bank = 0;
    auto block_reduce = [&](double v0, double v1, double v2, double v3, double v4, int op0, int op1, int op2, int op3, int op4) {
        double wv[5] = {v0, v1, v2, v3, v4};
        const int wop[5] = {op0, op1, op2, op3, op4};
        wave_reduce5(wv, wop);                // (stage by stage over the values: lsc_wave.hpp)
        const double r0 = wv[0], r1 = wv[1], r2 = wv[2], r3 = wv[3], r4 = wv[4];
        auto &bank = S.red[red_bank];         // [5][waves of the largest build]
        if (lane == 0) {
            bank[0][wave] = r0;
            if (op1 >= 0) bank[1][wave] = r1;
            if (op2 >= 0) bank[2][wave] = r2;
            if (op3 >= 0) bank[3][wave] = r3;
            if (op4 >= 0) bank[4][wave] = r4;
        }
        __syncthreads();
        const int nused = op4 >= 0 ? 5 : (op3 >= 0 ? 4 : (op2 >= 0 ? 3 : (op1 >= 0 ? 2 : 1)));
        double t = 0.0;
        {
            // (the partials of all waves in ONE batch of loads: read where they were combined they were a chain of four LDS round trips)
            const int ls = lane < nused ? lane : 0;
            const int op = ls == 0 ? op0 : (ls == 1 ? op1 : (ls == 2 ? op2 : (ls == 3 ? op3 : op4)));
            double bw[NWAVE];
#pragma unroll
            for (int w = 0; w < NWAVE; w++) bw[w] = bank[ls][w];
#pragma unroll
            for (int w = 0; w < NWAVE; w++) asm volatile("" : "+v"(bw[w]));
            t = bw[0];
#pragma unroll
            for (int w = 1; w < NWAVE; w++) t = op == 0 ? t + bw[w] : (op == 1 ? fmax(t, bw[w]) : fmin(t, bw[w]));
        }
        rv[0] = lane_value(t, 0);
        if (op1 >= 0) rv[1] = lane_value(t, 1);
        if (op2 >= 0) rv[2] = lane_value(t, 2);
        if (op3 >= 0) rv[3] = lane_value(t, 3);
        if (op4 >= 0) rv[4] = lane_value(t, 4);
        red_bank ^= 1;
    };
    // ... its sibling for the active-set solve's search: ONE value (the key, a maximum; rv[0]), and the chosen row's RECORD rides in rows 1-4 of
    // the same bank, which a one-value reduction leaves idle.  The key carries the row index, so exactly one lane of a wave holds the wave's
    // maximum: that lane stores its row's record into its wave's column -- word | 1 << 32 (0: "not published"), right-hand side, the three
    // components of an LSC row's normal -- in front of the barrier the reduction has anyway.  Behind it lane l loads entry l of the bank (row
    // l / NWAVE, column l % NWAVE: one load per lane where block_reduce has one per wave), the keys of lanes 0 .. NWAVE-1 are combined by DPP
    // (a maximum over the same values: the same bits in any order), and wave 0 reads the record of the winning wave's column from
    // the lanes that hold it.  The two-bank rule holds as for block_reduce: the next writer of this bank is the search after next.
    unsigned long long rec_w = 0ull;      // wave 0: the chosen row's word | published << 32
    double rec_h = 0.0;                   //         its right-hand side (AH(sl) | rrhs[r])
    float rec_n0 = 0.f, rec_n1 = 0.f, rec_n2 = 0.f;
    auto search_reduce = [&](unsigned long long key, bool with_record, bool pub, uint32_t word, double rhs, float n0, float n1, float n2) {
        double wv[5] = {__longlong_as_double((long long)key), 0.0, 0.0, 0.0, 0.0};
        const int wop[5] = {1, -1, -1, -1, -1};
        wave_reduce5(wv, wop);
        const double r0 = wv[0];
        auto &bank = S.red[red_bank];
        if (lane == 0) bank[0][wave] = r0;
        if (with_record && key != 0ull && key == (unsigned long long)__double_as_longlong(r0)) {
            bank[1][wave] = __longlong_as_double((long long)(pub ? (1ull << 32) | (unsigned long long)word : 0ull));
            bank[2][wave] = rhs;
            bank[3][wave] = __hiloint2double(__float_as_int(n1), __float_as_int(n0));
            bank[4][wave] = __hiloint2double(0, __float_as_int(n2));
        }
        __syncthreads();
        static_assert((NWAVE & (NWAVE - 1)) == 0 && NWAVE >= 2 && NWAVE <= 8 && 5 * NWAVE <= 64, "one bank entry per lane, a row of keys inside a DPP row");
        const int ls = lane < 5 * NWAVE ? lane : 0;
        double e = bank[ls / NWAVE][ls % NWAVE];
        asm volatile("" : "+v"(e));
        const int elo = __double2loint(e), ehi = __double2hiint(e);
        double v = e;
        int tlo = elo, thi = ehi;
#define LSC_STAGE(CTRL)                                                                                   \
        tlo = __builtin_amdgcn_update_dpp(tlo, __double2loint(v), CTRL, 0xf, 0xf, false);                 \
        thi = __builtin_amdgcn_update_dpp(thi, __double2hiint(v), CTRL, 0xf, 0xf, false);                 \
        v = hw_extreme<1>(v, __hiloint2double(thi, tlo));
        LSC_STAGE(0x111)
        if constexpr (NWAVE > 2) { LSC_STAGE(0x112) }
        if constexpr (NWAVE > 4) { LSC_STAGE(0x114) }
#undef LSC_STAGE
        rv[0] = lane_value(v, NWAVE - 1);      // (row_shr: lane NWAVE-1 holds the maximum of lanes 0 .. NWAVE-1; what lies above never moves down)
        if (with_record && wave == 0) {
            const long long km = __double_as_longlong(rv[0]);
            const unsigned long long hit = __ballot(lane < NWAVE && __double_as_longlong(e) == km);
            const int wi = __builtin_amdgcn_readfirstlane(hit != 0ull ? __ffsll((long long)hit) - 1 : 0);
            rec_w = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(ehi, NWAVE + wi) << 32) | (unsigned long long)(uint32_t)__builtin_amdgcn_readlane(elo, NWAVE + wi);
            rec_h = __hiloint2double(__builtin_amdgcn_readlane(ehi, 2 * NWAVE + wi), __builtin_amdgcn_readlane(elo, 2 * NWAVE + wi));
            rec_n0 = __int_as_float(__builtin_amdgcn_readlane(elo, 3 * NWAVE + wi));
            rec_n1 = __int_as_float(__builtin_amdgcn_readlane(ehi, 3 * NWAVE + wi));
            rec_n2 = __int_as_float(__builtin_amdgcn_readlane(elo, 4 * NWAVE + wi));
        }
        red_bank ^= 1;
    };

    // Reduction of the per-row values (w = z*t1 or 1, v = t2) into x-space weights and gradients.
    // Axis rows are gathered by the last 90 lanes, LSC buckets by units (bucket, component) from lane 0 up.
    auto reduce_rows = [&](bool with_w, bool unit_w) {
        if (tid >= NT - NV) {
            // Gather of the bound / velocity / acceleration rows that touch variable (k, t).  Slots that do not exist
            // (first control points, segment ends) keep s = 1, z = 0, t1 = t2 = 0 for the whole solve, so every load
            // below is unconditional and independent (no validity branches between them).
            const int k = xk, t = xt, i = t % NC;
            const int b = k * SEGV + t;
            const int t1i = t >= 1 ? t - 1 : 0, t2i = t >= 2 ? t - 2 : 0;
            const int o0 = k * SEGV + t, o1 = k * SEGV + t1i, o2 = k * SEGV + t2i;
            const double v0 = S.at2[0 * NV + o0], v1 = S.at2[1 * NV + o0], v2 = S.at2[2 * NV + o0], v3 = S.at2[3 * NV + o0];
            const double v4 = S.at2[4 * NV + o0], v5 = S.at2[5 * NV + o0];
            const double v2m = S.at2[2 * NV + o1], v3m = S.at2[3 * NV + o1], v4m = S.at2[4 * NV + o1], v5m = S.at2[5 * NV + o1];
            const double v4mm = S.at2[4 * NV + o2], v5mm = S.at2[5 * NV + o2];
            const double m1 = t >= 1 ? 1.0 : 0.0, m2 = t >= 2 ? 1.0 : 0.0;
            double g = (v0 - v1) + (v3 - v2) + (v4 - v5) + m1 * ((v2m - v3m) - 2.0 * (v4m - v5m)) + m2 * (v4mm - v5mm);
            double gzv = 0.0;
            double cg = cost_grad();   // this lane's (xk, xt) equal (k, t)
            if (i == DEG && t / NC >= M - S.tseg) cg += 2.0 * md.w_t * (S.x[b] - S.goal[k]);
            if (with_w) {
                double w0, w1, w2, w3, w4, w5, w2m, w3m, w4m, w5m, w4mm, w5mm;
                if (unit_w) {
                    // cold start: weight 1 on every existing row
                    w0 = AVALID(0 * NV + o0); w1 = AVALID(1 * NV + o0); w2 = AVALID(2 * NV + o0); w3 = AVALID(3 * NV + o0);
                    w4 = AVALID(4 * NV + o0); w5 = AVALID(5 * NV + o0);
                    w2m = AVALID(2 * NV + o1); w3m = AVALID(3 * NV + o1); w4m = AVALID(4 * NV + o1); w5m = AVALID(5 * NV + o1);
                    w4mm = AVALID(4 * NV + o2); w5mm = AVALID(5 * NV + o2);
                } else {
                    const double z0 = S.az[0 * NV + o0], z1 = S.az[1 * NV + o0], z2 = S.az[2 * NV + o0], z3 = S.az[3 * NV + o0];
                    const double z4 = S.az[4 * NV + o0], z5 = S.az[5 * NV + o0];
                    const double z2m = S.az[2 * NV + o1], z3m = S.az[3 * NV + o1], z4m = S.az[4 * NV + o1], z5m = S.az[5 * NV + o1];
                    const double z4mm = S.az[4 * NV + o2], z5mm = S.az[5 * NV + o2];
                    w0 = z0 * S.at1[0 * NV + o0]; w1 = z1 * S.at1[1 * NV + o0]; w2 = z2 * S.at1[2 * NV + o0]; w3 = z3 * S.at1[3 * NV + o0];
                    w4 = z4 * S.at1[4 * NV + o0]; w5 = z5 * S.at1[5 * NV + o0];
                    w2m = z2m * S.at1[2 * NV + o1]; w3m = z3m * S.at1[3 * NV + o1]; w4m = z4m * S.at1[4 * NV + o1]; w5m = z5m * S.at1[5 * NV + o1];
                    w4mm = z4mm * S.at1[4 * NV + o2]; w5mm = z5mm * S.at1[5 * NV + o2];
                    // stationarity residual (predictor passes only)
                    gzv = (z0 - z1) + (z3 - z2) + (z4 - z5) + m1 * ((z2m - z3m) - 2.0 * (z4m - z5m)) + m2 * (z4mm - z5mm);
                }
                const double wB = w0 + w1, wV0 = w2 + w3, wA0 = w4 + w5;
                const double wV1 = m1 * (w2m + w3m), wA1 = m1 * (w4m + w5m), wA2 = m2 * (w4mm + w5mm);
                S.W[W_D + b] = wB + wV0 + wV1 + wA0 + 4.0 * wA1 + wA2;
                S.W[W_1 + b] = -wV0 - 2.0 * wA0 - 2.0 * wA1;
                S.W[W_2 + b] = wA0;
            }
            S.gx[b] = cg + g;
            S.gz[b] = cg + gzv;
            if constexpr (PROF) { if (tid == NT - 1) t_acc[PH_RED_GATHER] += wall_clock64() - t_last; }
        }
        // LSC buckets: per control point  sum w n n^T (six components), -sum v n and -sum z n (three each; row vector a_r = -n).
        if constexpr (!SPILL) {
            // Row-major: one lane per slot = a few consecutive rows of one bucket; it loads each row once and accumulates all
            // twelve (corrector pass: six) components in registers -- about two instructions per product where one lane per
            // (bucket, component) spent ten -- and no lane waits for the fullest bucket (that wait was four fifths of this phase).
            // Partial sums go to LDS that is dead right now (see RSLOT_P); a second step adds the parts of a bucket in slot order.
            static_assert(offsetof(SmemT<!TABLES_IN_LDS>, dinv) - offsetof(SmemT<!TABLES_IN_LDS>, colbuf) >= sizeof(double) * RSLOT_C * 3,
                          "corrector-pass staging of the bucket sums");
            static_assert(RSLOT_P <= NT - NV && RSLOT_C <= NT - NV, "slot lanes and the axis-row gather lanes do not overlap");
            // (a corrector pass only needs -sum v n: the stationarity residual, which -sum z n feeds, is tested in predictor passes)
            const int ncomp = with_w ? 12 : 3;
            double *stage = with_w ? S.K : &S.colbuf[0][0];
            const unsigned short *soff = with_w ? S.soffP : S.soffC;
            if (tid < soff[NB]) {
                const uint32_t e = with_w ? S.slotP[tid] : S.slotC[tid];
                const int r0 = (int)(e & 0xffffu), n = (int)((e >> 16) & 0xffu);
                double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, t0 = 0, t1 = 0, t2 = 0, u0 = 0, u1 = 0, u2 = 0;
                // Two rows per trip, all twelve loads of the pair issued before anything waits (they used to sit behind the uniform
                // branches of the pass kind, one LDS round trip each: four per row).  An odd last row is read twice and its second copy
                // carries weight zero; the rows of a slot are still added in their order.
                for (int q = 0; q < n; q += 2) {
                    const int ra = r0 + q, rb = q + 1 < n ? ra + 1 : ra;
                    const bool two = q + 1 < n;
                    const float fax = rn[ra], fay = rn[R + ra], faz = rn[2 * R + ra], fbx = rn[rb], fby = rn[R + rb], fbz = rn[2 * R + rb];
                    const double va = rt2[ra], vb_ = rt2[rb], za_ = rz[ra], zb_ = rz[rb], ia = rt1[ra], ib = rt1[rb];
                    const double vb = two ? vb_ : 0.0, zb = two ? zb_ : 0.0;
                    {
                        const double nx = (double)fax, ny = (double)fay, nz = (double)faz;
                        t0 = fma(va, nx, t0); t1 = fma(va, ny, t1); t2 = fma(va, nz, t2);
                        if (with_w) {
                            u0 = fma(za_, nx, u0); u1 = fma(za_, ny, u1); u2 = fma(za_, nz, u2);
                            const double w = unit_w ? 1.0 : za_ * ia;
                            const double wx = w * nx, wy = w * ny, wz = w * nz;
                            s0 = fma(wx, nx, s0); s1 = fma(wx, ny, s1); s2 = fma(wx, nz, s2);
                            s3 = fma(wy, ny, s3); s4 = fma(wy, nz, s4); s5 = fma(wz, nz, s5);
                        }
                    }
                    {
                        const double nx = (double)fbx, ny = (double)fby, nz = (double)fbz;
                        t0 = fma(vb, nx, t0); t1 = fma(vb, ny, t1); t2 = fma(vb, nz, t2);
                        if (with_w) {
                            u0 = fma(zb, nx, u0); u1 = fma(zb, ny, u1); u2 = fma(zb, nz, u2);
                            const double w = two ? (unit_w ? 1.0 : zb * ib) : 0.0;
                            const double wx = w * nx, wy = w * ny, wz = w * nz;
                            s0 = fma(wx, nx, s0); s1 = fma(wx, ny, s1); s2 = fma(wx, nz, s2);
                            s3 = fma(wy, ny, s3); s4 = fma(wy, nz, s4); s5 = fma(wz, nz, s5);
                        }
                    }
                }
                double *o = stage + tid * ncomp;
                if (with_w) { o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3; o[4] = s4; o[5] = s5; o[9] = u0; o[10] = u1; o[11] = u2; o += 6; }
                o[0] = t0; o[1] = t1; o[2] = t2;
            }
            if constexpr (PROF) { if (tid == 0) t_acc[PH_RED_BUCKETS] += wall_clock64() - t_last; }
            __syncthreads();
            for (int o = tid; o < NB * ncomp; o += NT) {
                const int b = o / ncomp, c = o - b * ncomp, cp = b + 3;
                double sum = 0.0;
                for (int sl = soff[b]; sl < soff[b + 1]; sl++) {
                    double *e = stage + sl * ncomp + c;
                    sum += *e;
                    *e = 0.0;                                      // (K must not keep anything assemble() does not overwrite)
                }
                const int j = with_w ? c : c + 6;
                if (j < 6) S.W[W_S + cp * 6 + j] = sum;
                else if (j < 9) S.Tv[cp * 3 + (j - 6)] = -sum;
                else S.Tz[cp * 3 + (j - 9)] = -sum;
            }
        } else {
        // rows in HBM, up to 27 (N-1) of them: unit (bucket, c) loops over its bucket, c 0..5 -> sum w n n^T, 6..8 -> v n and z n
        // Two lanes per unit take the even / odd rows of the bucket and combine through a lane-pair shuffle.
        const int nunits = with_w ? NB * 9 : NB * 3;
        for (int ub = 0; ub < 2 * nunits; ub += NT) {      // one trip with 512 lanes, two with 256
            const int u = (ub + tid) >> 1, half = tid & 1;
            const bool live = u < nunits;
            const int bkt = live ? (with_w ? u / 9 : u / 3) : 0, c = live ? (with_w ? u % 9 : 6 + u % 3) : 6, cp = bkt + 3;
            // bucket base and size in one LDS word (offs | cnt << 16), written once after phase B
            int cnt, r0;
            if constexpr (SPILL) { cnt = live ? S.cnt[cp] : 0; r0 = S.offs[bkt]; }      // 27 (N-1) rows: may exceed 16 bits
            else { const uint32_t oc = live ? S.offcnt[bkt] : 0u; cnt = (int)(oc >> 16); r0 = (int)(oc & 0xffffu); }
            double acc0 = 0.0, acc1 = 0.0, az0 = 0.0, az1 = 0.0;
            if (c < 6) {
                const int ia = c < 3 ? 0 : (c < 5 ? 1 : 2), ib = c < 3 ? c : (c < 5 ? c - 2 : 2);
                const float *na = rn + ia * R + r0, *nb = rn + ib * R + r0;
                const double *pz = rz + r0, *pi = rt1 + r0;
                int j = half;
                for (; j + 2 < cnt; j += 4) {
                    const double a0 = (double)na[j] * (double)nb[j], a1 = (double)na[j + 2] * (double)nb[j + 2];
                    if (unit_w) { acc0 += a0; acc1 += a1; }
                    else { acc0 += pz[j] * pi[j] * a0; acc1 += pz[j + 2] * pi[j + 2] * a1; }
                }
                for (; j < cnt; j += 2) {
                    const double w = unit_w ? 1.0 : pz[j] * pi[j];
                    acc0 += w * (double)na[j] * (double)nb[j];
                }
            } else {
                const float *nc = rn + (c - 6) * R + r0;
                const double *pv = rt2 + r0, *pz = rz + r0;
                int j = half;
                for (; j + 2 < cnt; j += 4) {
                    const double n0 = (double)nc[j], n1 = (double)nc[j + 2];
                    acc0 += pv[j] * n0; acc1 += pv[j + 2] * n1;
                    az0 += pz[j] * n0; az1 += pz[j + 2] * n1;
                }
                for (; j < cnt; j += 2) { acc0 += pv[j] * (double)nc[j]; az0 += pz[j] * (double)nc[j]; }
            }
            double sa = acc0 + acc1, sz = az0 + az1;
            sa += __shfl_xor(sa, 1, 64);
            sz += __shfl_xor(sz, 1, 64);
            if (live && half == 0) {
                if (c < 6) S.W[W_S + cp * 6 + c] = sa;
                else { S.Tv[cp * 3 + (c - 6)] = -sa; S.Tz[cp * 3 + (c - 6)] = -sz; }
            }
        }
        }
        if constexpr (PROF && SPILL) { if (tid == 0) t_acc[PH_RED_BUCKETS] += wall_clock64() - t_last; }
        __syncthreads();
    };

    // K (lower band) from W ;  rhs = -Z^T (gx + Tv)
    auto assemble = [&](bool with_k) {
        if (with_k) {
            for (int e = tid; e < n_entries; e += NT) {
                const uint32_t id = ent[2 * e], t0 = ent[2 * e + 1], t1 = ent[2 * e + 3];
                double v;
                v = kconst[e];
                // four terms per trip: the term words first, then the weights they point at (two LDS round trips per trip instead of
                // two per term); terms past the entry's end get coefficient zero
                for (uint32_t q = t0; q < t1; q += 4) {
                    uint32_t tm[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) tm[u] = terms[q + u < t1 ? q + u : t0];
                    LSC_PIN(PV(tm[0]), PV(tm[1]), PV(tm[2]), PV(tm[3]));      // (the four words in one batch, then the four weights in one)
                    double w[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) w[u] = S.W[(tm[u] >> 8) & 0x3ff];
                    LSC_PIN(PV(w[0]), PV(w[1]), PV(w[2]), PV(w[3]));
#pragma unroll
                    for (int u = 0; u < 4; u++) v += (q + u < t1 ? (double)((int)(tm[u] & 0xff) - 128) : 0.0) * w[u];
                }
                S.K[(id >> 16) * KLD + (id & 0xffff)] = v;
            }
        }
        if (tid < NY) {
            const uint32_t yo = S.yop[tid], yp = S.ypp[tid];
            const int yo0 = yo & 0xff, yo1 = (yo >> 8) & 0xff, yo2 = (yo >> 16) & 0xff, yo3 = yo >> 24;
            const int yp0 = yp & 0xff, yp1 = (yp >> 8) & 0xff, yp2 = (yp >> 16) & 0xff, yp3 = yp >> 24;
            const double yc0 = S.ytc[tid][0], yc1 = S.ytc[tid][1], yc2 = S.ytc[tid][2], yc3 = S.ytc[tid][3];
            double r = yc0 * (S.gx[yo0] + S.Tv[yp0]) + yc1 * (S.gx[yo1] + S.Tv[yp1]) + yc2 * (S.gx[yo2] + S.Tv[yp2]) +
                       yc3 * (S.gx[yo3] + S.Tv[yp3]);
            S.rhs[tid] = -r;
            // projected stationarity residual Z^T (grad + A^T z), parked in dy (free until the solve)
            S.dy[tid] = yc0 * (S.gz[yo0] + S.Tz[yp0]) + yc1 * (S.gz[yo1] + S.Tz[yp1]) + yc2 * (S.gz[yo2] + S.Tz[yp2]) +
                        yc3 * (S.gz[yo3] + S.Tz[yp3]);
        }
        // (no barrier here: rhs and the parked residual are written by lanes of wave 0 and next read by wave 0 -- the stationarity
        // reduction, the substitutions --; K, written by everybody, is read behind the barrier of that reduction, or behind the
        // explicit one of the cold start)
    };

    // The factor lives in LDS (S.K, unit-diagonal M = L D^-1, lower band) between phases; registers hold it only inside
    // factor() and solve(), so the row passes and reductions in between keep the whole register budget.
    auto factor = [&]() -> bool {
        constexpr int RV = NY - 1;
        double lrow[NY];          // lane = row, register = column (wave 1: of the index-reversed matrix)
        int npos = 0;             // positive pivots of this wave's sweeps
        const double pend0[BAND] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        // Lane-dependent predicates are what this function avoids (round 4, read off the ISA: ~300 of them -- load masks, store masks, "lane == J"
        // selects -- were loop invariants of the solver loop, kept in scalar pairs, spilled into vector lanes and restored with two v_readlane
        // each, a fifth of the instructions of the factorisation's tail and of the substitutions):
        //  * loads: S.K holds zeros wherever it does not hold a band entry -- set once at entry, kept by the row reduction's staging (which
        //    clears what it parks there) and by assemble() (band entries only) --, so "outside the band" and "above the diagonal" read as 0.0;
        //  * the registers ABOVE a lane's diagonal collect meaningless updates (the symmetric half, started from zero); they feed nothing that
        //    is kept, so the hand-over of the middle block adds and stores whole rows, and only the write-back of T is masked -- by one compare
        //    per entry on an opaque copy of the lane index (so that it is not hoisted), instead of three spilled conditions.
        int rel = lane - 1;       // (lane - 1) - j in [0, BAND)  <=>  j < lane <= j + BAND
        asm volatile("" : "+v"(rel));
        if (wave < 2) {
            const int lk = lane < NY ? lane : NY - 1;      // (lanes beyond the matrix repeat the last row; nothing of theirs is kept)
            if (wave == 0) {
#pragma unroll
                for (int j = 0; j < NY; j++) lrow[j] = S.K[lk * KLD + j];
            } else {
                // K'[r][c] = K[RV-c][RV-r]; the middle block (and what lies beyond it) starts at zero: it only collects
                // the Schur updates of this sweep
#pragma unroll
                for (int j = 0; j < NY; j++) lrow[j] = j < TW_B ? S.K[(RV - j) * KLD + (RV - lk)] : 0.0;
            }
            double *const dinv_w = wave == 0 ? S.dinv : S.dinvb;
            // (wave 0 takes TW_A pivots from the top, wave 1 TW_B from the bottom: the same number, or one less when NY - BAND is odd)
            if constexpr (TW_A == TW_B) chol_step<0, TW_A>(lrow, S.colbuf[wave], dinv_w, lane, npos, 0.0, pend0, 0.0, pend0);      // (one body for both waves)
            else if (wave == 0) chol_step<0, TW_A>(lrow, S.colbuf[wave], dinv_w, lane, npos, 0.0, pend0, 0.0, pend0);
            else chol_step<0, TW_B>(lrow, S.colbuf[wave], dinv_w, lane, npos, 0.0, pend0, 0.0, pend0);
            if (wave == 1) {
                // the middle block in the reversed numbering is [TW_B, TW_B + BAND); reversed (r, c) is original (RV - r, RV - c)
                if (lane >= TW_B && lane < TW_B + BAND) {
#pragma unroll
                    for (int c = TW_B; c < TW_B + BAND; c++) S.mid2[(RV - c - TW_A) * BAND + (RV - lane - TW_A)] = lrow[c];
                }
                if (lane == 0) S.ok2 = npos == TW_B ? 1.0 : 0.0;
            }
        }
        __syncthreads();
        if (wave == 0) {
            if (lane >= TW_A && lane < TW_M1) {
#pragma unroll
                for (int k = TW_A; k < TW_M1; k++) lrow[k] += S.mid2[(lane - TW_A) * BAND + (k - TW_A)];
            }
            if (lane >= TW_M1) {
#pragma unroll
                for (int k = TW_A; k < TW_M1; k++) lrow[k] = 0.0;      // rows below the middle block belong to the other sweep
            }
            chol_step<TW_A, TW_M1>(lrow, S.colbuf[0], S.dinv, lane, npos, 0.0, pend0, 0.0, pend0);
            if (lane < TW_M1) {
#pragma unroll
                for (int j = 0; j < TW_M1; j++)
                    if ((unsigned)(rel - j) < (unsigned)BAND) S.K[lane * KLD + j] = lrow[j];
                S.K[lane * KLD + lane] = 0.0;      // (the diagonal of K: the substitutions read rows and columns of T unmasked)
            }
            if (lane == 0) S.sc[7] = npos == TW_M1 ? 1.0 : 0.0;
        } else if (wave == 1) {
            // multipliers of the bottom-up sweep, reversed (r, c) -> original (RV-r, RV-c), kept at the mirrored band position
#pragma unroll
            for (int c = 0; c < TW_B; c++)
                if ((unsigned)(rel - c) < (unsigned)BAND) S.K[(RV - c) * KLD + (RV - lane)] = lrow[c];
            if (lane < TW_B) S.K[(RV - lane) * KLD + (RV - lane)] = 0.0;
        }
        __syncthreads();
        return S.sc[7] != 0.0 && S.ok2 != 0.0;
    };
    // T D T^T dy = rhs on wave 0 alone (round 3; it ran on two waves with three workgroup barriers and two LDS hand-overs, 2.8 us:
    // the chains below are as long, but nothing waits for another wave).  lane = unknown.  Every step broadcasts one component
    // (two v_readlane) and takes coefficient x component off the lanes that follow it in the elimination order; the coefficients
    // -- entries of T in LDS, zero where the band ends -- do not depend on the chain and are loaded ahead of it.  The top-down
    // and the bottom-up sweep touch different lanes: they run as two independent chains (two accumulators) side by side.
    auto solve = [&]() {
        constexpr int RV = NY - 1;
        if (wave == 0) {
            const int l = lane;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // rhs was written by this wave (assemble): wave-level order is enough
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // The loads are unconditional (what a lane outside the range reads lies inside this struct and is discarded) and pinned
            // group by group (pin_values), so that a group is ONE batch of loads ahead of its chain.
            const int lr = l < NY ? l : NY - 1;
            const double *Krow = S.K + lr * KLD;            // T[l][.]
            const double *Kcol = S.K + lr;                  // T[.][l]
            const double rhs = l < NY ? S.rhs[l] : 0.0;
            const double dinv = l < TW_M1 ? S.dinv[l] : S.dinvb[l < NY ? RV - l : 0];
            double bt = l < TW_M1 ? rhs : 0.0;              // top-down sweep: unknowns 0..13, what it takes off the middle rows
            double bb = l >= TW_M1 ? rhs : 0.0;             // bottom-up sweep: unknowns 38..25, what it takes off the middle rows
            {
                double ct[TW_A], cb[TW_B];
#pragma unroll
                for (int q = 0; q < TW_A; q++) ct[q] = Krow[q];
#pragma unroll
                for (int q = 0; q < TW_B; q++) cb[q] = Kcol[(RV - q) * KLD];
                pin_values(ct);
                pin_values(cb);
                // (no masks: T[l][q] for l outside (q, q + BAND] and T[RV - q][l] for l outside [RV - q - BAND, RV - q) are zeros of S.K --
                //  above the diagonal, the zeroed diagonal, outside the band; see factor())
#pragma unroll
                for (int q = 0; q < TW_A; q++) {
                    // both broadcasts first, in scalar pairs of their own, then both updates: with one pair reused for the two chains every
                    // update sat one wait state behind its v_readlane (VALU-writes-SGPR hazard), 27 s_nop per solve on the wave that issues alone
                    double xt = lane_value(bt, q), xb = q < TW_B ? lane_value(bb, RV - (q < TW_B ? q : 0)) : 0.0;
                    asm volatile("" : "+s"(xt), "+s"(xb));
                    bt = fma(-ct[q], xt, bt);
                    if (q < TW_B) bb = fma(-cb[q < TW_B ? q : 0], xb, bb);
                }
            }
            double b = bt + bb;
            {
                double cm[BAND - 1];
#pragma unroll
                for (int q = 0; q < BAND - 1; q++) cm[q] = Krow[TW_A + q];
                pin_values(cm);
                // (rows below the middle block hold the other sweep's multipliers in these columns: they sit this block out)
                double bm = b;
#pragma unroll
                for (int q = 0; q < BAND - 1; q++) bm = fma(-cm[q], lane_value(bm, TW_A + q), bm);
                b = l < TW_M1 ? bm : b;
            }
            b *= dinv;
            {   // back: the middle block first (its solution goes to the rows above AND below it), then outwards
                double cu[BAND], cd[BAND];
#pragma unroll
                for (int q = 0; q < BAND; q++) { const int I = TW_M1 - 1 - q; cu[q] = Kcol[I * KLD]; cd[q] = Krow[I]; }
                pin_values(cu);
                pin_values(cd);
                const bool below = l >= TW_M1;
#pragma unroll
                for (int q = 0; q < BAND; q++) cu[q] = below ? cd[q] : cu[q];      // T[I][l]: rows above I (middle and top: the column, zero from the
                                                                                   // diagonal on) | a bottom row l: its entry at the mirrored place, T[l][I]
#pragma unroll
                for (int q = 0; q < BAND; q++) b = fma(-cu[q], lane_value(b, TW_M1 - 1 - q), b);
            }
            bt = b; bb = b;
            {
                double co[TW_A - 1], ci[TW_B - 1];
#pragma unroll
                for (int q = 0; q < TW_A - 1; q++) co[q] = Kcol[(TW_A - 1 - q) * KLD];
#pragma unroll
                for (int q = 0; q < TW_B - 1; q++) ci[q] = Krow[TW_M1 + q];
                pin_values(co);
                pin_values(ci);
#pragma unroll
                for (int q = 0; q < TW_A - 1; q++) {
                    double xt = lane_value(bt, TW_A - 1 - q), xb = q < TW_B - 1 ? lane_value(bb, TW_M1 + (q < TW_B - 1 ? q : 0)) : 0.0;
                    asm volatile("" : "+s"(xt), "+s"(xb));
                    bt = fma(-co[q], xt, bt);
                    if (q < TW_B - 1) bb = fma(-ci[q < TW_B - 1 ? q : 0], xb, bb);
                }
            }
            if (l < NY) S.dy[l] = l < TW_M1 ? bt : bb;
            if constexpr (PROF) { if (tid == 0) t_acc[PH_SPARE0] += wall_clock64() - t_last; }
            compute_x_wave0(S.dy, S.dx, false);      // dx right here, on the wave that holds dy (one workgroup barrier less per solve)
        }
        __syncthreads();
    };
    // LSC row helpers (row r: -n.x <= -rhs)
    auto lsc_ax = [&](const double *xv, int r, int cp) -> double {
        return -((double)rn[r] * xv[cp] + (double)rn[R + r] * xv[SEGV + cp] + (double)rn[2 * R + r] * xv[2 * SEGV + cp]);
    };

    int status = LSC_STATUS_INFEASIBLE_K;
    int iters = 0;
    double obj = 0.0;
    const double hmax = fmax(1.0, fmax(fabs((double)md.world_max[0]), fabs((double)md.world_min[0])));

    // The solver is a small state machine so that the (fully unrolled, register-heavy) factorisation and triangular
    // solves exist at exactly one place in the code:
    //   ST_COLD : cold start  (H + A^T A) y = -grad(x0) + A^T (h - A x0), then s, z shifted into the interior
    //   ST_PRED : residuals at the current point, Hessian, factorisation, affine (predictor) direction
    //   ST_CORR : corrector right-hand side, same factor, combined direction, step
    // Start: warm (y = free control points of the shifted previous plan, every row centred on mu0) when enabled,
    // with the cold start as fallback; cold only otherwise.
    enum { ST_COLD = 0, ST_PRED = 1, ST_CORR = 2, ST_START_WARM = 3, ST_START_COLD = 4 };      // (the last two: the next pass of the loop prepares that start first)
    int phase = ST_PRED, attempt = md.ws_mu0 > 0.0 ? 0 : 1, spent = 0;
    double alpha = 1.0, gap = 0.0, rpmax = 0.0, mu = 0.0, smu = 0.0, tau = 0.99;
    bool gap_ok = false;
    const int max_iters = md.max_iters;

    auto prepare_cold = [&]() {
        if (tid < 40) S.y[tid] = 0.0;
        __syncthreads();
        compute_x(S.y, S.x, true);
        __syncthreads();
        for (int c = tid; c < n_ax; c += NT) {
            const uint32_t am = S.amap[c]; const int sl = am & 1023, type = (am >> 10) & 7, ak = (am >> 13) & 3, at = am >> 15;
            S.at2[sl] = ax_row(S.x, type, ak, at) - AH(sl);
        }
        for (int c = tid; c < nact; c += NT) {
            const uint32_t e = cmap[c];
            const int r = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
            rt2[r] = lsc_ax(S.x, r, cp) + rrhs[r];
        }
        __syncthreads();
    };
    auto prepare_warm = [&](double mu0) {
        if (tid < NY) {
            const int g = tid, k = yaxis(g), va = yvar(g);
            const int t = va < NYL ? (va / 3) * NC + 3 + (va % 3) : (M - 1) * NC + 3;
            S.y[g] = (dim2 && k == 2) ? md.z2d : (double)S.pinit[k * SEGV + t];
        }
        __syncthreads();
        compute_x(S.y, S.x, true);
        __syncthreads();
        const double smin = sqrt(mu0);
        for (int c = tid; c < n_ax; c += NT) {
            const uint32_t am = S.amap[c]; const int sl = am & 1023, type = (am >> 10) & 7, ak = (am >> 13) & 3, at = am >> 15;
            // velocity / acceleration rows are stored divided by n/dt and n(n-1)/dt^2: scale the floor with them so that
            // the start equals the one of the reference's row scaling
            const double floor_s = type < 2 ? smin : (type < 4 ? smin * md.hv_scale : smin * md.ha_scale);
            const double sv = fmax(AH(sl) - ax_row(S.x, type, ak, at), floor_s);
            S.as_[sl] = sv; S.az[sl] = mu0 / sv; S.at1[sl] = 0.0; S.at2[sl] = 0.0;
        }
        for (int c = tid; c < nact; c += NT) {
            const uint32_t e = cmap[c];
            const int r = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
            const double sv = fmax(-rrhs[r] - lsc_ax(S.x, r, cp), smin);
            rs[r] = sv; rz[r] = mu0 / sv; rt1[r] = 0.0; rt2[r] = 0.0;
        }
        __syncthreads();
    };

    // ---------------------------------------------------------------- dual active set (SOLVER == 1)
    // Goldfarb & Idnani (1983) on the 39-unknown reduced problem  min 1/2 y'Hy + g'y  s.t.  G y <= h,  started from the unconstrained
    // optimum with an empty working set: the most violated row is added (after dropping the rows whose multipliers the step would
    // take below zero) until nothing is violated.  Why it pays here: measured on the CPU over six missions (tests/prototypes/
    // active_set_study.py, profiles/r05_active_set_study.log) the optimum holds at most 9 active rows of the ~2 000, and the agent a
    // tick waits for needs 8 changes of the working set in the median and 13 at the 99th percentile -- against 9-12 interior-point
    // iterations of ~17 us.  A change costs one pass over the rows (the search for the most violated one) and a few dozen
    // dependent operations on wave 0.  What keeps it small: the reduced Hessian is the SAME 13 x 13 block for every axis, agent and
    // tick up to the number of terminal segments, so its inverse comes from the host (Model::ginv); the working set is capped at
    // GQ rows, the inverse of its Gram matrix S = G_W H^-1 G_W' is updated per change (q <= 12).  Anything unusual -- more than GQ active rows,
    // more than GI_CAP changes, a Gram matrix that is not positive definite (dependent rows), no admissible step (an infeasible
    // QP) -- returns false and the interior point decides, as before.
    constexpr int HV = (NYA * NYA + 7) & ~7;
    constexpr int GI_CAP = 60;
    int gi_changes = 0;
    bool gi_infeasible = false;          // the active-set solve proved the QP infeasible (see "no admissible step")
    auto gi_solve = [&]() -> bool {
        if constexpr (SOLVER != 1) return false;
        else {
        double *const gk = S.K;                       // the interior point's K is idle until then (re-zeroed on the way there)
        double *const Yw = gk;                        // [GQ][GS] H^-1 times the rows of the working set (y-space)
        double *const Si = Yw + GQ * GS;              // [GQ][GQ] inverse of the Gram matrix G_W H^-1 G_W'
        double *const uw = Si + GQ * GQ;              // [GQ] multipliers
        double *const rwv = uw + GQ;                  // [GQ] multiplier rates of the current step
        int *const wrow = reinterpret_cast<int *>(rwv + GQ);   // [GQ] row codes (index into amap, or n_ax + index into cmap)
        static_assert(GQ * GS + GQ * GQ + 2 * GQ + (GQ + 1) / 2 <= NY * KLD, "the working set fits the idle K");
        double *const gyv = S.gz;                     // [40], idle here
        // gi_hz[t][a] = (H^-1 Z' e_t)_a for the variable t of an axis (SEGV x NYA, the same for the three axes): H^-1 times a row's normal is
        // then three of these per lane instead of a 13-term product behind an LDS round trip.  Kept in the interior point's idle slack array
        // S.as_ (AXROWS >= SEGV * NYA doubles; set back to 1.0 on the way to the interior point).
        double *const gi_hz = S.as_;
        double *const gi_zt = S.az;                   // Z itself, laid out the same way (Model::gzt): a row's normal in y-space by the same lookup
        static_assert(SEGV * NYA <= AXROWS, "gi_hz fits the slack array");
        const double INF = 1e300;
        // (early: everything up to the first search except the scales of the LSC rows stands in LDS since barrier (3))
        if (!early) {
#pragma unroll
        for (int u = 0; u < GI_NPRE; u++) if (tid + u * NT < SEGV * NYA) { gi_hz[tid + u * NT] = gi_pre_z[u]; gi_zt[tid + u * NT] = gi_pre_n[u]; }
        }
        // Selection scale of every row, 1 / (1 + |right-hand side|), formed ONCE per solve (it was two divisions per lane in every search:
        // ~80 of a search's ~190 instructions per wave); a row inside the working set carries scale 0 -- its mark: it can never be the most
        // violated one.  Kept in the interior point's idle t2 arrays (S.at2, rt2; ip_late_setup / prepare_* rewrite both on the way there).
        // (hardware reciprocal + Newton: the scale only ranks violations, an ulp is nothing to it -- a division is ~40 instructions)
        if (!early) for (int c = tid; c < n_ax; c += NT) { const int sl = S.amap[c] & 1023; S.at2[sl] = rcp_nr(1.0 + fabs(AH(sl))); }
        // (early: no barrier between these stores and the first search -- cmap[c] & CMAP_MASK == c, so every reader of a scale in front of the
        //  search's block reduction is the lane that wrote it.  A lane without an LSC row of its own -- tid >= nact -- reads slot 0 there,
        //  rt2[0] and rrhs[0], possibly while lane 0 stores rt2[0]: that value never leaves the lane, `s_has_l` masks it out of the search.)
        for (int c = tid; c < nact; c += NT) { const int r = cmap[c] & CMAP_MASK; rt2[r] = rcp_nr(1.0 + fabs(rrhs[r])); }
        if (!early) {
        for (int i = tid; i < GQ * GS + GQ * GQ + 2 * GQ; i += NT) Yw[i] = 0.0;      // Yw, Si, uw, rwv: rows beyond the working set meet zeros
        // unconstrained optimum y = -H^-1 Z' grad(x0): a linear map of this axis' state constants and goal coordinate, its matrix from the host
        if (tid < 40) {
            const int k = tid < NY ? yaxis(tid) : 0;
            double yv = gi_pre_y[0] * S.s0[k][0] + gi_pre_y[1] * S.s0[k][1] + gi_pre_y[2] * S.s0[k][2] + gi_pre_y[3] * S.goal[k];
            if (dim2 && k == 2) yv = md.z2d;          // planar world: z is not a variable (src/traj_optimizer.cpp:264-266): no cost, no rows, y_z rests at z_2d
            S.y[tid] = tid < NY ? yv : 0.0;
        }
        __syncthreads();
        }
        int q = 0;
        // (wave 0 alone keeps qhw, the largest working set of this solve: it sizes the step's loops, see "SIZE CLASS" below)
        int qhw = 0;
        const bool all_slots = a.step_all_slots != 0;      // LSC_STEP_ALL_SLOTS: every change in class GQ
        const bool row_record = a.plain_handover == 0;     // LSC_SOLVE_ROW_RECORD; the default: the step loads the chosen row itself
        int *const gi_code = reinterpret_cast<int *>(&S.sc[0]);      // the step's code, the one word a step publishes (0: go on)
        // (diagnostics: lsc_working_set_peaks; GQ + 1 = the solve gave up for want of a slot)
        auto peak_out = [&]() { if (a.ws_peak && tid == 0) a.ws_peak[qi] = qhw; };
        // x from y on wave 0 (variables lane and lane + 64), with what never changes during the solve -- the y-indices and coefficients of the two
        // variables, their state constants -- held in registers: one batch of six loads of y per call
        const int xv0 = lane, xv1 = lane + 64 < NV ? lane + 64 : lane;
        const uint32_t xg0 = S.xgp[xv0], xg1 = S.xgp[xv1];
        const double xa00 = S.xtc[xv0 % SEGV][0], xa01 = S.xtc[xv0 % SEGV][1], xa02 = S.xtc[xv0 % SEGV][2];
        const double xa10 = S.xtc[xv1 % SEGV][0], xa11 = S.xtc[xv1 % SEGV][1], xa12 = S.xtc[xv1 % SEGV][2];
        const bool xs0 = xv0 % SEGV < 3, xs1 = xv1 % SEGV < 3;
        const double xk0 = xs0 ? X0C(xv0) : 0.0, xk1 = xs1 ? X0C(xv1) : 0.0;
        auto gi_x = [&]() { gi_x_lanes(xv0, xv1, xg0, xg1, xa00, xa01, xa02, xa10, xa11, xa12, xs0, xs1, xk0, xk1); };
        if (!early) {
            if (wave == 0) gi_x();
            __syncthreads();
        }
        stamp(PH_INIT);                  // (instrumented build: the start of the active-set solve is booked under "ip_init")
        // What the search needs of this lane's first axis row and first LSC row never changes during the solve: kept in registers, so that a
        // search is ONE batch of loads (the point and the two scales) instead of row word -> row data -> value.
        const bool s_has_ax = tid < n_ax, s_has_l = tid < nact;
        const uint32_t s_am = S.amap[s_has_ax ? tid : 0];
        const int s_sl = s_am & 1023, s_type = (s_am >> 10) & 7, s_xo = (int)((s_am >> 13) & 3) * SEGV + (int)(s_am >> 15);
        const double s_hh = AH(s_sl);
        const uint32_t s_e = s_has_l ? cmap[tid] : 0u;
        const int s_r = s_e & CMAP_MASK, s_cp = s_e >> CMAP_SHIFT;
        const double s_lh = rrhs[s_r];
        const float s_n0 = rn[s_r], s_n1 = rn[R + s_r], s_n2 = rn[2 * R + s_r];
        for (;;) {
            // (S.x is current: formed by wave 0 right behind the step that changed y, in front of the barrier that ended it)
            // ---- the most violated row outside the working set (violation over 1 + |right-hand side|; ties: lowest row)
            double best = 0.0;
            int bidx = 0;
            double lv = 0.0;
            {
                double sc = S.at2[s_sl], x0 = S.x[s_xo], x1 = S.x[s_xo + 1], x2 = S.x[s_xo + 2];
                double lsc_ = rt2[s_r], p0 = S.x[s_cp], p1 = S.x[SEGV + s_cp], p2 = S.x[2 * SEGV + s_cp];
                // (the code of the step that ended the last round rides in the same batch: one wait, then the branch.  The step publishes this
                //  ONE word; q and gi_changes never leave wave 0, whose lane 0 writes every output they go into)
                int stepped = *gi_code;
                LSC_PIN(PV(sc), PV(x0), PV(x1), PV(x2), PV(lsc_), PV(p0), PV(p1), PV(p2), PV(stepped));
                stepped = __builtin_amdgcn_readfirstlane(stepped);
                if (stepped != 0) { gi_infeasible = stepped == 3; peak_out(); return false; }
                const double v = (ax_row3(x0, x1, x2, s_type) - s_hh) * sc;
                if (s_has_ax && v > best) { best = v; bidx = tid; }
                lv = (s_lh - ((double)s_n0 * p0 + (double)s_n1 * p1 + (double)s_n2 * p2)) * lsc_;
            }
            for (int c = tid + NT; c < n_ax; c += NT) {
                const uint32_t am = S.amap[c]; const int sl = am & 1023, type = (am >> 10) & 7, ak = (am >> 13) & 3, at = am >> 15;
                const double *xq = S.x + ak * SEGV + at;
                double sc = S.at2[sl], x0 = xq[0], x1 = xq[1], x2 = xq[2], hh = AH(sl);
                LSC_PIN(PV(sc), PV(x0), PV(x1), PV(x2), PV(hh));
                const double v = (ax_row3(x0, x1, x2, type) - hh) * sc;
                if (v > best) { best = v; bidx = c; }
            }
            if (s_has_l && lv > best) { best = lv; bidx = n_ax + tid; }
            for (int c = tid + NT; c < nact; c += NT) {
                const uint32_t e = cmap[c];
                const int r = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
                double sc = rt2[r], x0 = S.x[cp], x1 = S.x[SEGV + cp], x2 = S.x[2 * SEGV + cp], hh = rrhs[r];
                float n0 = rn[r], n1 = rn[R + r], n2 = rn[2 * R + r];
                LSC_PIN(PV(sc), PV(x0), PV(x1), PV(x2), PV(hh), PV(n0), PV(n1), PV(n2));
                const double v = (hh - ((double)n0 * x0 + (double)n1 * x1 + (double)n2 * x2)) * sc;
                if (v > best) { best = v; bidx = n_ax + c; }
            }
            // one reduction: violation as float32 bits in the upper word, ~row in the lower -- as a double it orders like the pair
            const unsigned long long key = best > 0.0 ? (((unsigned long long)__float_as_uint((float)best)) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)bidx) : 0ull;
            // ... and the lane that holds the chosen row hands the step what it knows of it (search_reduce: the row's record).  Only the
            // register-resident first rows are published; a best row out of the `c += NT` loops goes as "not published" and the step loads it.
            const bool pub_ax = bidx < n_ax;
            const bool pub = pub_ax ? bidx == tid : bidx == n_ax + tid;
            search_reduce(key, row_record, pub, pub_ax ? s_am : s_e, pub_ax ? s_hh : s_lh, s_n0, s_n1, s_n2);
            const unsigned long long kmax = (unsigned long long)__double_as_longlong(rv[0]);
            stamp(PH_P1);                // ("residual_pass": x from y and the search for the most violated row)
            if (!(__uint_as_float((uint32_t)(kmax >> 32)) > 1e-10f)) break;                  // nothing violated: optimal
            const int idx = (int)(0xffffffffu - (uint32_t)(kmax & 0xffffffffull));
            if (wave == 0) {
                // ---- the step, on wave 0 alone.  A lone wave hides no latency: every LDS round trip costs its ~100 cycles in full, so the
                // step is laid out as FOUR batches of independent loads, each waited for once (the first version -- loads where they were
                // used, a Cholesky factor with two substitutions, guards on a working-set size the compiler held in a vector register -- made
                // ~30 round trips and ~850 instructions: 2.7 us per change; profiles/r05_step_rewrite.log).
                q = __builtin_amdgcn_readfirstlane(q);        // (uniform by construction; in a scalar register the guards below are scalar branches)
                // batch 1: the row's word -> three x-variables with their coefficients
                // (t, k: each variable's index inside its axis and its axis.  They are carried from where v is formed -- v = k * SEGV + t with
                //  0 <= t < SEGV on both paths, an axis row never leaves its axis -- so that no v % SEGV, v / SEGV runs on the lone wave)
                int v0, v1, v2, t0, t1, t2, k0, k1, k2, rsl = 0;
                double a0, a1, a2, hp;
                // (conditions that are the same on every lane by construction are SAID to be: the compiler takes anything derived from an LDS
                //  load for divergent and builds exec-mask branches and loops around it)
                auto uni = [](bool b_) { return __builtin_amdgcn_readfirstlane((int)b_) != 0; };
                const bool is_ax = idx < n_ax;
                // (the row's record, when the search published one: word, right-hand side and normal are scalars, and no trip to LDS stands in
                //  front of batch 2.  Otherwise -- the default; under LSC_SOLVE_ROW_RECORD a row out of the search's `c += NT` loops -- the word is loaded
                //  here, and right-hand side and normal travel WITH batch 2: one wait for both, where there were two)
                const bool have = row_record && (rec_w >> 32) != 0ull;
                uint32_t word;
                if (have) word = (uint32_t)rec_w;
                else word = is_ax ? S.amap[idx] : cmap[idx - n_ax];
                if (is_ax) {
                    const uint32_t am = word; const int sl = am & 1023, type = (am >> 10) & 7, ak = (am >> 13) & 3, at = am >> 15;
                    const int kind = type >> 1;
                    const double sg = (type & 1) ? -1.0 : 1.0;
                    a0 = sg * (kind == 1 ? -1.0 : 1.0); a1 = sg * (kind == 0 ? 0.0 : (kind == 1 ? 1.0 : -2.0)); a2 = sg * (kind == 2 ? 1.0 : 0.0);
                    v0 = ak * SEGV + at; v1 = kind >= 1 ? v0 + 1 : v0; v2 = kind == 2 ? v0 + 2 : v0;
                    t0 = at; t1 = kind >= 1 ? at + 1 : at; t2 = kind == 2 ? at + 2 : at;
                    k0 = k1 = k2 = ak;
                    rsl = sl;
                } else {
                    const uint32_t e = word;
                    const int r = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
                    v0 = cp; v1 = SEGV + cp; v2 = 2 * SEGV + cp;
                    t0 = t1 = t2 = cp;
                    k0 = 0; k1 = 1; k2 = 2;
                    rsl = r;
                    a0 = a1 = a2 = 0.0;
                }
                // batch 2: right-hand side, normal, the point, the variables' y-indices and coefficients, and this lane's entries of
                // H^-1 Z' e_v (gi_hz: one table for every axis, built at the start of the solve)
                const int lk = lane < NY ? yaxis(lane) : 3, lva = lane < NY ? yvar(lane) : 0;
                // (the loads of the fallback are unconditional -- an axis row reads slot 0 of the normals -- and nothing is formed from them in
                //  front of the pin: a sign or a select here would wait for them on their own)
                double hh;
                float n0, n1, n2;
                if (have) { hh = rec_h; n0 = rec_n0; n1 = rec_n1; n2 = rec_n2; }
                else {
                    const int rl = is_ax ? 0 : rsl;
                    if constexpr (TABLES_IN_LDS) hh = *(is_ax ? &S.ah[rsl] : &rrhs[rsl]);
                    else hh = is_ax ? AH(rsl) : rrhs[rsl];
                    n0 = rn[rl]; n1 = rn[R + rl]; n2 = rn[2 * R + rl];
                }
                double x0 = S.x[v0], x1 = S.x[v1], x2 = S.x[v2];
                uint32_t gp0 = S.xgp[v0], gp1 = S.xgp[v1], gp2 = S.xgp[v2];
                double c00 = S.xtc[t0][0], c01 = S.xtc[t0][1], c02 = S.xtc[t0][2], c10 = S.xtc[t1][0], c11 = S.xtc[t1][1], c12 = S.xtc[t1][2],
                       c20 = S.xtc[t2][0], c21 = S.xtc[t2][1], c22 = S.xtc[t2][2];
                double h0 = gi_hz[t0 * NYA + lva], h1 = gi_hz[t1 * NYA + lva], h2 = gi_hz[t2 * NYA + lva];
                double z0 = gi_zt[t0 * NYA + lva], z1 = gi_zt[t1 * NYA + lva], z2 = gi_zt[t2 * NYA + lva];
                LSC_PIN(PV(x0), PV(x1), PV(x2), PV(gp0), PV(gp1), PV(gp2), PV(c00), PV(c01), PV(c02), PV(c10), PV(c11), PV(c12), PV(c20), PV(c21), PV(c22),
                        PV(h0), PV(h1), PV(h2), PV(z0), PV(z1), PV(z2), PV(hh), PV(n0), PV(n1), PV(n2));
                hp = is_ax ? hh : -hh;             // (an LSC row -n.x <= -rhs)
                if (!is_ax) { a0 = -(double)n0; a1 = -(double)n1; a2 = -(double)n2; }
                double viol = a0 * x0 + a1 * x1 + a2 * x2 - hp;
                // the row's normal in y-space and H^-1 times it: this lane's entries of Z' e_v and of H^-1 Z' e_v for the row's three variables
                // (lanes beyond the unknowns have lk = 3: both stay zero)
                const double m0 = lk == k0 ? a0 : 0.0, m1 = lk == k1 ? a1 : 0.0, m2 = lk == k2 ? a2 : 0.0;
                const double np_g = m0 * z0 + m1 * z1 + m2 * z2;
                double hin_g = m0 * h0 + m1 * h1 + m2 * h2;
                if (dim2 && lk == 2) hin_g = 0.0;            // (planar world: the z unknowns never move)
                double up = 0.0;
                int code = 0;
                // The INVERSE of the Gram matrix S = G_W H^-1 G_W' is kept across changes (Si, q x q, lane i holds row i): the multiplier rates
                // r = S^-1 d are then GQ multiply-adds per lane with d_j read from lane j (v_readlane) -- no dependent chain beyond that --, a
                // row that joins borders the inverse ([S d; d' nu]^-1 = [Si + r r'/delta, -r/delta; -r'/delta, 1/delta], delta = nu - d'r, the
                // Schur complement = the slope of the new row along the step), a row that leaves removes its row and column (Si' = A - b b'/c).
                // What a Cholesky factor had and this has not -- backward stability when rows are nearly dependent -- is bounded by the test
                // on delta below and caught by the verification pass behind the solve: either way the interior point decides.
                // Rows / columns beyond q hold zeros or stale finite numbers and meet r_j = d_j = 0: the loops run unguarded -- over the QC
                // slots of a SIZE CLASS (4, 8 or GQ), the smallest that covers qhw, the largest working set this solve has held so far; the
                // classes are instantiations of the one body below (loop bounds stay constants, Sr / Yc / rb / Tn register arrays with static
                // indices), picked by a scalar branch per change.  Why the slots j in [QC, GQ) can be left out without changing a bit:
                //  * they lie at or beyond qhw, and nothing was ever stored there: Yw[j][.], Si[.][j], Si[j][.] hold the +0.0 of the solve's
                //    start, and rwv[j] = d_j = +0.0 (both are masked by `lane < q`, q <= qhw);
                //  * the terms of r left out are fma(+0, +0, rw) = rw: the sum starts at +0.0 and a sum is -0.0 only if both operands are,
                //    so rw is never -0.0 and adding +0.0 keeps it;
                //  * the terms of z left out are fma(-(+0), +0, zg) = zg + (-0.0) = zg for every zg, -0.0 included;
                //  * the stores of the bordered inverse left out would write fma(rs_, +0, +0) = +0.0 (rs_ is finite: delta passed its test)
                //    over +0.0 -- on a full step at q == qhw too: column q gets its -rs_ by a store of its own behind the loop;
                //  * Tn[k] is only stored for k < q.
                // A class by q instead would NOT be exact: slots in [q, qhw) hold stale values after a drop, (-Yc) * (+0) can be +0.0 there
                // and turns a zg of -0.0 into +0.0 -- an agent of a circle swap on a coordinate axis has such exact zeros.
                // (a.step_all_slots -- LSC_STEP_ALL_SLOTS, tests and A/B runs -- holds every change to class GQ.)
                const int lq = lane < GQ ? lane : GQ - 1, lg = lane < GS ? lane : GS - 1;
                auto change = [&](auto qc_) -> bool {          // one change of the working set in class QC; true: the step is over
                    constexpr int QC = decltype(qc_)::value;
                    static_assert(QC <= GQ, "a class is a prefix of the working set's slots");
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    // batch 3: everything the working set contributes
                    double Sr[QC], Yc[QC];                      // row `lane` of the inverse; entry `lane` of every H^-1 n_w
                    const double *yr = Yw + lq * GS;
                    double y00 = yr[gp0 & 0xff], y01 = yr[(gp0 >> 8) & 0xff], y02 = yr[gp0 >> 16], y10 = yr[gp1 & 0xff], y11 = yr[(gp1 >> 8) & 0xff], y12 = yr[gp1 >> 16],
                           y20 = yr[gp2 & 0xff], y21 = yr[(gp2 >> 8) & 0xff], y22 = yr[gp2 >> 16];
#pragma unroll
                    for (int j = 0; j < QC; j++) { Sr[j] = Si[lq * GQ + j]; Yc[j] = Yw[j * GS + lg]; }
                    double uwl = uw[lq], yl = S.y[lg];
                    LSC_PIN(PV(y00), PV(y01), PV(y02), PV(y10), PV(y11), PV(y12), PV(y20), PV(y21), PV(y22), PV(uwl), PV(yl));
                    pin_values(Sr);
                    pin_values(Yc);
                    // d = G_W H^-1 n = Y_W n, with the (at most nine) non-zeros of n
                    double dw = a0 * (c00 * y00 + c01 * y01 + c02 * y02) + a1 * (c10 * y10 + c11 * y11 + c12 * y12) + a2 * (c20 * y20 + c21 * y21 + c22 * y22);
                    dw = lane < q ? dw : 0.0;
                    double rw = 0.0;
#pragma unroll
                    for (int j = 0; j < QC; j++) rw = fma(Sr[j], lane_value(dw, j), rw);          // r = S^-1 d
                    rw = lane < q ? rw : 0.0;
                    // r to every lane through LDS (one store, one batch of broadcast loads): read lane by lane it was 4 issue slots per entry,
                    // twice (the direction here, the update of the inverse below)
                    if (lane < GQ) rwv[lane] = rw;
                    double rb[QC];
#pragma unroll
                    for (int w = 0; w < QC; w++) rb[w] = rwv[w];
                    pin_values(rb);
                    // primal direction z = H^-1 n - Y_W r (it keeps the working set active) and its slope against the new row
                    double zg = hin_g;
#pragma unroll
                    for (int w = 0; w < QC; w++) zg = fma(-Yc[w], rb[w], zg);
                    zg = lane < NY ? zg : 0.0;
                    // one staged reduction for the three wave-wide numbers of a step: n'H^-1 n, the slope n'z, the smallest multiplier ratio
                    const double ratio = (lane < q && rw > 1e-13) ? uwl * rcp_nr(rw) : INF;
                    double red4[5] = {np_g * hin_g, np_g * zg, ratio, 0.0, 0.0};
                    const int rop[5] = {0, 0, 2, -1, -1};
                    wave_reduce5(red4, rop);
                    const double nph = red4[0], zn = red4[1], t1 = red4[2];
                    const unsigned long long dropmask = __ballot(lane < q && ratio == t1);
                    const double t2 = zn > 1e-12 * nph ? viol * rcp_nr(zn) : INF;
                    if (uni(t1 >= INF && t2 >= INF)) {
                        // No admissible step: the new row is a non-negative combination of working-set rows pointing the other way -- the rows
                        // contradict each other (Farkas), the QP is infeasible.  With a violation that is not round-off (> 1e-6 of the row's
                        // scale) the verdict is final: code 3, status 1, no interior-point run (an infeasible agent used to cost the tick the
                        // ~26 iterations of two diverging interior-point starts); a marginal one is left to the interior point like every
                        // other irregularity.
                        code = uni(viol > 1e-6 * (1.0 + fabs(hp))) ? 3 : 1;
                        return true;
                    }
                    const double t = fmin(t1, t2);
                    if (uni(t2 < INF)) {
                        if (lane < NY) S.y[lane] = yl - t * zg;
                        viol -= t * zn;
                    }
                    if (lane < q) uw[lane] = fmax(uwl - t * rw, 0.0);
                    up += t;
                    gi_changes++;
                    if (uni(t2 <= t1)) {
                        // full step: the row joins the working set; the inverse is bordered with (r, delta), delta = n'H^-1 n - d'r -- which IS the
                        // slope n'z of the new row along the step (z = H^-1 n - Y_W r), already reduced: no reduction of its own
                        if (uni(q == GQ)) { code = 2; qhw = GQ + 1; return true; }
                        const double delta = zn;
                        if (uni(!(delta > 1e-11 * nph))) { code = 2; return true; }
                        const double idl = rcp_nr(delta);
                        if (lane < GS) Yw[q * GS + lane] = hin_g;
                        const double rs_ = rw * idl;
#pragma unroll
                        for (int j = 0; j < QC; j++) Sr[j] = fma(rs_, rb[j], Sr[j]);
                        if (lane < q) {
#pragma unroll
                            for (int j = 0; j < QC; j++) Si[lane * GQ + j] = Sr[j];
                            Si[lane * GQ + q] = -rs_;
                            Si[q * GQ + lane] = -rs_;
                        }
                        if (lane == 0) {
                            Si[q * GQ + q] = idl; uw[q] = up; wrow[q] = idx;
                            if (is_ax) S.at2[rsl] = 0.0;            // (scale 0 = inside the working set)
                            else rt2[rsl] = 0.0;
                        }
                        q = __builtin_amdgcn_readfirstlane(q + 1);
                        qhw = __builtin_amdgcn_readfirstlane(q > qhw ? q : qhw);
                        return true;
                    }
                    // partial step: row jd of the working set reached multiplier zero and leaves (the last row takes its place)
                    const int jd = __builtin_amdgcn_readfirstlane(__ffsll((long long)dropmask) - 1), last = q - 1;
                    if (lane == 0) {
                        const int code_j = wrow[jd];
                        if (code_j < n_ax) { const int sl = S.amap[code_j] & 1023; S.at2[sl] = rcp_nr(1.0 + fabs(AH(sl))); }
                        else { const int r = cmap[code_j - n_ax] & CMAP_MASK; rt2[r] = rcp_nr(1.0 + fabs(rrhs[r])); }
                    }
                    {
                        // inverse without row / column jd:  T = A - b b' / c  (c = Si[jd][jd], b = column jd), then row / column `last` -> jd
                        const double cjj = Si[jd * GQ + jd];
                        const double bi = Si[lq * GQ + jd] * (1.0 / cjj);
                        double Tn[QC];
#pragma unroll
                        for (int k = 0; k < QC; k++) Tn[k] = fma(-bi, Si[jd * GQ + k], Sr[k]);
                        pin_values(Tn);
                        if (lane < q && lane != jd) {
                            const int ir = lane == last ? jd : lane;
#pragma unroll
                            for (int k = 0; k < QC; k++) {
                                if (k < q && k != jd) Si[ir * GQ + (k == last ? jd : k)] = Tn[k];
                            }
                        }
                    }
                    if (uni(jd != last)) {
                        if (lane < GS) Yw[jd * GS + lane] = Yw[last * GS + lane];
                        if (lane == 0) { uw[jd] = uw[last]; wrow[jd] = wrow[last]; }
                    }
                    q = __builtin_amdgcn_readfirstlane(q - 1);
                    gi_changes = __builtin_amdgcn_readfirstlane(gi_changes);
                    if (uni(gi_changes > GI_CAP)) { code = 2; return true; }
                    return false;
                };
                for (;;) {
                    const int qn = all_slots ? GQ : qhw;          // (scalar: the class is a scalar branch)
                    bool over;
                    if (qn <= 4) over = change(std::integral_constant<int, 4>());
                    else if (qn <= 8 || GQ <= 8) over = change(std::integral_constant<int, GQ < 8 ? GQ : 8>());
                    else over = change(std::integral_constant<int, GQ>());
                    if (over) break;
                }
                if (uni(code == 3)) {
                    // The verdict is final (no interior-point run behind it), so the certificate is evaluated once more from the rows themselves: with
                    // n = G_W' r, r <= 0, every feasible point has n'y >= sum_j r_j h_j, and the QP is infeasible iff that exceeds h_p -- which at ANY
                    // point x equals (a_p'x - h_p) - sum_j r_j (a_j'x - h_j).  Formed at the x of the current y with fresh residuals of the working
                    // rows: rows that drifted off their boundaries (the kept inverse is never refactorised) show up here, and the agent goes to the
                    // interior point like every other irregularity.
                    gi_x();
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    auto residual = [&](int rc) -> double {
                        if (rc < n_ax) {
                            const uint32_t am = S.amap[rc]; const int sl = am & 1023, type = (am >> 10) & 7, ak = (am >> 13) & 3, at = am >> 15;
                            const double *xq = S.x + ak * SEGV + at;
                            return ax_row3(xq[0], xq[1], xq[2], type) - AH(sl);
                        }
                        const uint32_t e = cmap[rc - n_ax];
                        const int r = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
                        return rrhs[r] - ((double)rn[r] * S.x[cp] + (double)rn[R + r] * S.x[SEGV + cp] + (double)rn[2 * R + r] * S.x[2 * SEGV + cp]);
                    };
                    const double rj = lane < q ? rwv[lane] : 0.0;
                    const double part = lane < q ? rj * residual(wrow[lane]) : 0.0;
                    const double gap = residual(idx) - wave_sum(part);
                    if (uni(!(gap > 0.5e-6 * (1.0 + fabs(hp))))) code = 1;
                }
                if (lane == 0) *gi_code = code;
                if (code == 0) gi_x();               // x for the next search, on the wave that holds the new y
            }
            __syncthreads();
            stamp(PH_FACTOR);            // ("cholesky": the step on wave 0 -- normal, direction, ratio test, update of the working set)
        }
        // Nothing outside the working set is violated.  The rows INSIDE it were made active when they joined and every later step kept
        // them active -- up to the accuracy of the Gram solve: with nearly dependent rows they can drift, and a marked row is never
        // looked at again above.  So every row is checked once more, marks ignored; a violation here hands the agent to the interior point.
        // (Only the rows inside the working set can fail this -- the search that ended the loop formed the same residual times the same scale
        //  from this very S.x for every other row, and its maximum, as a float32, was not above 1e-10f, a tenth of the 1e-9 asked for here.  A
        //  check of wrow[0 .. q) alone, one lane of wave 0 each, was built and measured: not faster -- three dependent LDS trips on one wave
        //  against two that eight waves hide -- and dropped: profiles/step_size_classes_ab.log.)
        {
            double worst = 0.0;
            for (int c = tid; c < n_ax; c += NT) {
                const uint32_t am = S.amap[c]; const int sl = am & 1023, type = (am >> 10) & 7, ak = (am >> 13) & 3, at = am >> 15;
                const double *xq = S.x + ak * SEGV + at;
                double x0 = xq[0], x1 = xq[1], x2 = xq[2], hh = AH(sl);
                LSC_PIN(PV(x0), PV(x1), PV(x2), PV(hh));
                worst = fmax(worst, (ax_row3(x0, x1, x2, type) - hh) * rcp_nr(1.0 + fabs(hh)));
            }
            for (int c = tid; c < nact; c += NT) {
                const uint32_t e = cmap[c];
                const int r = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
                double x0 = S.x[cp], x1 = S.x[SEGV + cp], x2 = S.x[2 * SEGV + cp], hh = rrhs[r];
                float n0 = rn[r], n1 = rn[R + r], n2 = rn[2 * R + r];
                LSC_PIN(PV(x0), PV(x1), PV(x2), PV(hh), PV(n0), PV(n1), PV(n2));
                worst = fmax(worst, (hh - ((double)n0 * x0 + (double)n1 * x1 + (double)n2 * x2)) * rcp_nr(1.0 + fabs(hh)));
            }
            // the objective at S.x (formed at the top of the last round) rides on the same block reduction: like the interior point's residual pass
            double objp = 0.0;
            if (tid < NV && !(dim2 && xk == 2)) {          // (planar world: the cost runs over `k < dim`, src/traj_optimizer.cpp:330, 367)
                objp = 0.5 * cost_grad() * S.x[tid];
                if (xterm) { const double e = S.x[tid] - S.goal[xk]; objp += md.w_t * e * e; }
            }
            block_reduce(worst, objp, 0.0, 0.0, 0.0, 1, 0, -1, -1, -1);
            peak_out();
            if (rv[0] > 1e-9) return false;
            obj = rv[1];
        }
        stamp(PH_P2);                    // ("affine_pass": the verification pass and the objective)
        return true;
        }
    };

    bool run = true, run_gi_done = false;
    if (a.goal_err && a.goal_err[qi] != 0) {
        status = LSC_STATUS_GOAL_K;  // the goal planner ran out of LDS capacity: no goal, no plan
        run = false;
    } else if (a.sfc_err && a.sfc_err[qi] != 0) {
        status = LSC_STATUS_SFC_K;   // seed box of the corridor blocked (the reference throws out of plan())
        run = false;
    } else if (ALT && S.gen) {
        status = LSC_STATUS_GENERAL_K;   // solved by lsc_general_kernel, launched right after this one
        run = false;
    } else if (overflow) {
        status = LSC_STATUS_CAPACITY_K;
        run = false;
    } else if (SOLVER == 1 && gi_solve() && a.solver != 2) {      // (solver 2: test mode -- the solve runs and hands EVERY agent over)
        status = LSC_STATUS_OK_K;        // the active-set solve reached the optimum: obj and S.x are set
        iters = gi_changes;
        run = false;
        run_gi_done = true;
    } else if (SOLVER == 1 && gi_infeasible && a.solver != 2) {
        status = LSC_STATUS_INFEASIBLE_K;    // proved by the active-set solve: the stale plan is kept (src/traj_planner.cpp:1553-1584)
        iters = gi_changes;
        run = false;
        run_gi_done = true;
    } else {
        if constexpr (SOLVER == 1) {
            // the active-set solve gave up: the interior point starts from its own initial state (K zero outside the band, no marks)
            // ip_late_setup: the state the interior point expects at its start, built here instead of on every agent's way to the active-set solve
            ip_ytables();
            if constexpr (TABLES_IN_LDS) {
                uint32_t *lt = S.dyn, *le = lt + ((n_terms + 1) & ~1);
                for (int i = tid; i < n_terms; i += NT) lt[i] = a.terms[i];
                for (int i = tid; i < 2 * n_entries + 2; i += NT) le[i] = a.entries[i];
            }
            for (int i = tid; i < NY * KLD; i += NT) S.K[i] = 0.0;
            // (S.as_ held gi_hz, S.at2 the selection scales; slots of rows that do not exist keep s = 1, z = t1 = t2 = 0 for the whole solve)
            for (int i = tid; i < AXROWS; i += NT) { S.as_[i] = 1.0; S.az[i] = 0.0; S.at1[i] = 0.0; S.at2[i] = 0.0; }
            for (int i = tid; i < NCP * 3; i += NT) { S.Tv[i] = 0.0; S.Tz[i] = 0.0; }
            for (int i = tid; i < W_SIZE; i += NT) S.W[i] = 0.0;
            if (tid < 40) { S.y[tid] = 0.0; S.dy[tid] = 0.0; }
            if (tid < 64) {
                const int which = tid >> 5, b = tid & 31;
                slot_offsets(which, b, b < NB ? S.cnt[b + 3] : 0, nact);
            }
            spent = gi_changes;          // (reported with the iterations, like the iterations of a failed warm start)
            // A handed-over agent goes straight to the COLD start: what the active-set solve gives up on -- a working set beyond its capacity, an
            // infeasible QP -- is what the warm start (shifted previous plan, every row centred) fails on too, and its failed attempt was half of
            // the hand-over's cost (configs[3], tools/forest_stats.py: 26 -> 16 interior-point iterations per hand-over, plan kernel 0.51 -> 0.34 ms
            // with static goals, 0.28 -> 0.17 ms with grid goals).
            // ... but the cold start is NOT the last word on a verdict (round 6, found by the M = 4 fuzzer at seed 9500131): on a QP whose feasible
            // set is tiny it can run into its divergence test where the warm start -- and the oracle -- converge.  attempt 2: cold first, and
            // when THAT fails the warm start gets the second opinion the cold start used to give it (only agents whose cold start fails pay).
            attempt = md.ws_mu0 > 0.0 ? 2 : 1;
            __syncthreads();
            for (int e = tid; e < n_entries; e += NT) kconst[e] = kconst_of(ent[2 * e]);
            slot_entries();
            __syncthreads();
        }
    }
    // (one call site per start: the second opinion below re-enters here through the phase)
    phase = attempt == 0 ? ST_START_WARM : ST_START_COLD;
    if (!run) stamp(PH_INIT);

    while (run) {
        if (phase >= ST_START_WARM) {
            if (phase == ST_START_WARM) {
                // An agent with few surviving LSC rows (most agents of a sparse swarm) is close to its unconstrained optimum: it
                // starts a third as far from the boundary.  Over 36 missions this takes 10 % off the ticks of random swarms and
                // leaves crossing swarms where they were (profiles/r02_solver_knob_sweeps.log).  Not in corridor worlds: there the
                // box rows, which this count does not see, are what is active (the 256-agent forest loses 2.6 % with the rule).
                prepare_warm((nact < WS_FEW_ROWS && !md.use_sfc) ? md.ws_mu0 * (1.0 / 3.0) : md.ws_mu0);
                phase = ST_PRED;
            } else {
                prepare_cold();
                phase = ST_COLD;
            }
            stamp(PH_INIT);
        }
        bool failed = false;
        // ---------------------------------------------------------------- before the linear solve
        if (phase == ST_PRED) {
            if (iters >= max_iters) failed = true;
            else {
                // P1 (fused with the previous step): s += alpha ds, z += alpha dz, then residuals, 1/s, v = w rp
                double gp = 0.0, rpm = 0.0;
                for (int c = tid; c < n_ax; c += NT) {
                    const uint32_t am = S.amap[c]; const int sl = am & 1023, type = (am >> 10) & 7, ak = (am >> 13) & 3, at = am >> 15;
                    const double *xq = S.x + ak * SEGV + at;
                    double l_s = S.as_[sl], l_ds = S.at1[sl], l_z = S.az[sl], l_dz = S.at2[sl], x0 = xq[0], x1 = xq[1], x2 = xq[2], hh = AH(sl);
                    LSC_PIN(PV(l_s), PV(l_ds), PV(l_z), PV(l_dz), PV(x0), PV(x1), PV(x2), PV(hh));
                    double sv = l_s + alpha * l_ds, zv = l_z + alpha * l_dz;
                    double rp = ax_row3(x0, x1, x2, type) + sv - hh;
                    double is = 1.0 / sv;
                    S.as_[sl] = sv; S.az[sl] = zv;
                    S.at1[sl] = is;
                    S.at2[sl] = zv * is * rp;
                    gp += sv * zv; rpm = fmax(rpm, fabs(rp));
                }
                for (int c = tid; c < nact; c += NT) {
                    const uint32_t e = cmap[c];
                    const int r = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
                    double l_s = rs[r], l_ds = rt1[r], l_z = rz[r], l_dz = rt2[r], x0 = S.x[cp], x1 = S.x[SEGV + cp], x2 = S.x[2 * SEGV + cp], hh = rrhs[r];
                    float n0 = rn[r], n1 = rn[R + r], n2 = rn[2 * R + r];
                    LSC_PIN(PV(l_s), PV(l_ds), PV(l_z), PV(l_dz), PV(x0), PV(x1), PV(x2), PV(hh), PV(n0), PV(n1), PV(n2));
                    double sv = l_s + alpha * l_ds, zv = l_z + alpha * l_dz;
                    double rp = -((double)n0 * x0 + (double)n1 * x1 + (double)n2 * x2) + sv + hh;
                    double is = 1.0 / sv;
                    rs[r] = sv; rz[r] = zv;
                    rt1[r] = is;
                    rt2[r] = zv * is * rp;
                    gp += sv * zv; rpm = fmax(rpm, fabs(rp));
                }
                // objective: sum x'(w_c Q)x + w_t sum |c - g|^2  (src/traj_optimizer.cpp:329-372)
                double objp = 0.0;
                if (tid < NV && !(dim2 && xk == 2)) {      // (planar world: the cost runs over `k < dim`, :330, 367)
                    objp = 0.5 * cost_grad() * S.x[tid];
                    if (xterm) { double e = S.x[tid] - S.goal[xk]; objp += md.w_t * e * e; }
                }
                block_reduce(gp, rpm, objp, 0.0, 0.0, 0, 1, 0, -1, -1);
                gap = rv[0]; rpmax = rv[1]; obj = rv[2];
                mu = gap / nrow;
                gap_ok = gap <= md.gap_tol * (1.0 + fabs(obj));
                if (tid == 0) { S.sc[5] = gap; S.sc[6] = rpmax; }
                stamp(PH_P1);
                if (!(gap == gap) || !(rpmax == rpmax)) failed = true;
                // Divergence: on an infeasible QP the multipliers run away and the gap grows without bound; a convergent
                // run never exceeds its starting gap by orders of magnitude.  Stop this start instead of burning the
                // iteration cap (the cold start still gets its turn, and decides).
                if (iters == 0) { if (tid == 0) S.gap0 = gap; }
                else if (gap > 1e8 * S.gap0) failed = true;
            }
        } else if (phase == ST_CORR) {
            // P3: corrector right-hand side  v = w rp - (ds dz - sigma mu)/s
            for (int c = tid; c < n_ax; c += NT) {
                const uint32_t am = S.amap[c]; const int sl = am & 1023, type = (am >> 10) & 7, ak = (am >> 13) & 3, at = am >> 15;
                const double *xq = S.x + ak * SEGV + at;
                double sv = S.as_[sl], zv = S.az[sl], is = S.at1[sl], cc = S.at2[sl], x0 = xq[0], x1 = xq[1], x2 = xq[2], hh = AH(sl);
                LSC_PIN(PV(sv), PV(zv), PV(is), PV(cc), PV(x0), PV(x1), PV(x2), PV(hh));
                double rp = ax_row3(x0, x1, x2, type) + sv - hh;
                S.at2[sl] = zv * is * rp - (cc - smu) * is;
            }
            for (int c = tid; c < nact; c += NT) {
                const uint32_t e = cmap[c];
                const int r = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
                double sv = rs[r], zv = rz[r], is = rt1[r], cc = rt2[r], x0 = S.x[cp], x1 = S.x[SEGV + cp], x2 = S.x[2 * SEGV + cp], hh = rrhs[r];
                float n0 = rn[r], n1 = rn[R + r], n2 = rn[2 * R + r];
                LSC_PIN(PV(sv), PV(zv), PV(is), PV(cc), PV(x0), PV(x1), PV(x2), PV(hh), PV(n0), PV(n1), PV(n2));
                double rp = -((double)n0 * x0 + (double)n1 * x1 + (double)n2 * x2) + sv + hh;
                rt2[r] = zv * is * rp - (cc - smu) * is;
            }
            __syncthreads();
            stamp(PH_P3);
        }
        if (!failed) {
            const bool with_w = phase != ST_CORR;
            reduce_rows(with_w, phase == ST_COLD);
            stamp(PH_REDUCE);
            assemble(with_w);
            if (phase == ST_COLD) __syncthreads();
            stamp(PH_ASSEMBLE);
            if (phase == ST_PRED) {
                // cheap exit before the factorisation: primal residual, gap and stationarity all at tolerance
                const double rda = (tid < NY) ? fabs(S.dy[tid]) : 0.0;
                block_reduce(rda, 0.0, 0.0, 0.0, 0.0, 1, -1, -1, -1, -1);
                if (rpmax <= 1e-9 * hmax && gap_ok && rv[0] <= 1e-5 * (1.0 + fabs(obj))) { status = LSC_STATUS_OK_K; break; }
            }
            if (with_w) {
                const bool fok = factor();
                stamp(PH_FACTOR);
                if (!fok) {
                    if (a.trace && qi == a.trace_agent && tid == 0 && iters < 64) { double *tr = a.trace + iters * 8; tr[0] = gap; tr[1] = rpmax; tr[2] = obj; tr[3] = -1; tr[5] = -1; tr[7] = mu; }
                    // K lost definiteness to round-off: accept only a point that is already optimal to slightly relaxed
                    // tolerances -- primal residual, gap AND the projected stationarity residual (rv[0], reduced just
                    // above for the cheap exit); otherwise this start has failed
                    if (phase == ST_PRED && rpmax <= 1e-8 * hmax && gap <= 1e-7 * (1.0 + fabs(obj)) &&
                        rv[0] <= 1e-5 * (1.0 + fabs(obj))) { status = LSC_STATUS_OK_K; break; }
                    failed = true;
                }
            }
        }
        if (!failed) {
            solve();
            stamp(PH_SOLVE);
            // ------------------------------------------------------------ after the linear solve
            if (phase == ST_COLD) {
                if (tid < NY) S.y[tid] = S.dy[tid];
                __syncthreads();
                compute_x(S.y, S.x, true);
                __syncthreads();
                double mins = 1e300, minz = 1e300;
                for (int c = tid; c < n_ax; c += NT) {
                    const uint32_t am = S.amap[c]; const int sl = am & 1023, type = (am >> 10) & 7, ak = (am >> 13) & 3, at = am >> 15;
                    double sv = AH(sl) - ax_row(S.x, type, ak, at);
                    S.as_[sl] = sv; S.az[sl] = -sv;
                    mins = fmin(mins, sv); minz = fmin(minz, -sv);
                }
                for (int c = tid; c < nact; c += NT) {
                    const uint32_t e = cmap[c];
                    const int r = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
                    double sv = -rrhs[r] - lsc_ax(S.x, r, cp);
                    rs[r] = sv; rz[r] = -sv;
                    mins = fmin(mins, sv); minz = fmin(minz, -sv);
                }
                block_reduce(mins, minz, 0.0, 0.0, 0.0, 2, 2, -1, -1, -1);
                const double shs = rv[0] <= 0.0 ? 1.0 - rv[0] : 0.0;
                const double shz = rv[1] <= 0.0 ? 1.0 - rv[1] : 0.0;
                // the shift enters the loop as a "step" of length 1 (t1 = ds, t2 = dz) applied by the first fused pass
                for (int c = tid; c < n_ax; c += NT) { const int sl = S.amap[c] & 1023; S.at1[sl] = shs; S.at2[sl] = shz; }
                for (int c = tid; c < nact; c += NT) { const int r = cmap[c] & CMAP_MASK; rt1[r] = shs; rt2[r] = shz; }
                __syncthreads();
                alpha = 1.0;
                phase = ST_PRED;
                stamp(PH_INIT);
            } else if (phase == ST_PRED) {
                // P2: affine step length and centring statistics (+ the Newton-step convergence test).
                // Ratio test without a division: along the affine direction s dz + z ds = -s z, so with r = ds / s (= ds * t1, t1 = 1 / s from
                // P1) the two ratios of a row are -ds / s = -r and -dz / z = 1 + r; the step is 1 / max(1, max over rows of both).  (Two
                // predicated fp64 divisions per row stood here: ~15 instructions each.)
                double rmax = 0.0, s1 = 0.0, s2 = 0.0;
                for (int c = tid; c < n_ax; c += NT) {
                    const uint32_t am = S.amap[c]; const int sl = am & 1023, type = (am >> 10) & 7, k = (am >> 13) & 3, t = am >> 15;
                    const double *xq = S.x + k * SEGV + t, *dq = S.dx + k * SEGV + t;
                    double sv = S.as_[sl], zv = S.az[sl], is = S.at1[sl], x0 = xq[0], x1 = xq[1], x2 = xq[2], hh = AH(sl), d0 = dq[0], d1 = dq[1], d2 = dq[2];
                    LSC_PIN(PV(sv), PV(zv), PV(is), PV(x0), PV(x1), PV(x2), PV(hh), PV(d0), PV(d1), PV(d2));
                    double w = zv * is;
                    double rp = ax_row3(x0, x1, x2, type) + sv - hh;
                    double adx = ax_row3(d0, d1, d2, type);
                    double ds = -rp - adx, dz = -zv - w * ds;
                    const double r = ds * is;
                    rmax = fmax(rmax, fmax(-r, 1.0 + r));
                    s1 += sv * dz + zv * ds; s2 += ds * dz;
                    S.at2[sl] = ds * dz;
                }
                for (int c = tid; c < nact; c += NT) {
                    const uint32_t e = cmap[c];
                    const int r_ = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
                    double sv = rs[r_], zv = rz[r_], is = rt1[r_], x0 = S.x[cp], x1 = S.x[SEGV + cp], x2 = S.x[2 * SEGV + cp], hh = rrhs[r_];
                    double d0 = S.dx[cp], d1 = S.dx[SEGV + cp], d2 = S.dx[2 * SEGV + cp];
                    float n0 = rn[r_], n1 = rn[R + r_], n2 = rn[2 * R + r_];
                    LSC_PIN(PV(sv), PV(zv), PV(is), PV(x0), PV(x1), PV(x2), PV(hh), PV(d0), PV(d1), PV(d2), PV(n0), PV(n1), PV(n2));
                    double w = zv * is;
                    double rp = -((double)n0 * x0 + (double)n1 * x1 + (double)n2 * x2) + sv + hh;
                    double adx = -((double)n0 * d0 + (double)n1 * d1 + (double)n2 * d2);
                    double ds = -rp - adx, dz = -zv - w * ds;
                    const double r = ds * is;
                    rmax = fmax(rmax, fmax(-r, 1.0 + r));
                    s1 += sv * dz + zv * ds; s2 += ds * dz;
                    rt2[r_] = ds * dz;
                }
                const double dxa = (tid < NV) ? fabs(S.dx[tid]) : 0.0, xa = (tid < NV) ? fabs(S.x[tid]) : 0.0;
                block_reduce(rmax, s1, s2, dxa, xa, 1, 0, 0, 1, 1);
                // Newton-step test: with gap and primal residual at tolerance, the affine (pure Newton) step measures
                // the distance to the optimum (the stationarity residual itself can stall at the round-off level of
                // the ill-conditioned normal equations when z/s is huge).
                if (rpmax <= 1e-9 * hmax && gap_ok && rv[3] <= md.dx_tol * fmax(1.0, rv[4])) { status = LSC_STATUS_OK_K; break; }
                const double aaff = 1.0 / fmax(rv[0], 1.0);
                const double mu_aff = (gap + aaff * rv[1] + aaff * aaff * rv[2]) / nrow;
                double sigma = mu > 0.0 ? mu_aff / mu : 0.0;
                sigma = md.sigma_pow == 2 ? sigma * sigma : (md.sigma_pow == 4 ? (sigma * sigma) * (sigma * sigma) : sigma * sigma * sigma);
                smu = sigma * mu;
                tau = fmin(1.0 - 1e-5, fmax(0.99, aaff));
                if (a.trace && qi == a.trace_agent && tid == 0 && iters < 64) {
                    double *tr = a.trace + iters * 8;
                    tr[0] = gap; tr[1] = rpmax; tr[2] = obj; tr[3] = aaff; tr[4] = sigma; tr[6] = rv[3]; tr[7] = mu;
                }
                phase = ST_CORR;
                stamp(PH_P2);
            } else {
                // P4: step length; the step itself stays in t1 = ds, t2 = dz for the fused pass of the next round.
                // (ratio test as max of -ds / s = -ds * t1 and -dz / z = -dz * (1 / z), reciprocal by v_rcp_f64 + one Newton step; one division
                //  per workgroup behind the reduction instead of two predicated ones per row)
                double rmax = 0.0;
                for (int c = tid; c < n_ax; c += NT) {
                    const uint32_t am = S.amap[c]; const int sl = am & 1023, type = (am >> 10) & 7, k = (am >> 13) & 3, t = am >> 15;
                    const double *xq = S.x + k * SEGV + t, *dq = S.dx + k * SEGV + t;
                    double sv = S.as_[sl], zv = S.az[sl], is = S.at1[sl], cc = S.at2[sl], x0 = xq[0], x1 = xq[1], x2 = xq[2], hh = AH(sl), d0 = dq[0], d1 = dq[1], d2 = dq[2];
                    LSC_PIN(PV(sv), PV(zv), PV(is), PV(cc), PV(x0), PV(x1), PV(x2), PV(hh), PV(d0), PV(d1), PV(d2));
                    double w = zv * is;
                    double rp = ax_row3(x0, x1, x2, type) + sv - hh;
                    double adx = ax_row3(d0, d1, d2, type);
                    double ds = -rp - adx, dz = -zv + cc + w * adx;
                    rmax = fmax(rmax, fmax(-ds * is, -dz * rcp_nr(zv)));
                    S.at1[sl] = ds; S.at2[sl] = dz;
                }
                for (int c = tid; c < nact; c += NT) {
                    const uint32_t e = cmap[c];
                    const int r = e & CMAP_MASK, cp = e >> CMAP_SHIFT;
                    double sv = rs[r], zv = rz[r], is = rt1[r], cc = rt2[r], x0 = S.x[cp], x1 = S.x[SEGV + cp], x2 = S.x[2 * SEGV + cp], hh = rrhs[r];
                    double d0 = S.dx[cp], d1 = S.dx[SEGV + cp], d2 = S.dx[2 * SEGV + cp];
                    float n0 = rn[r], n1 = rn[R + r], n2 = rn[2 * R + r];
                    LSC_PIN(PV(sv), PV(zv), PV(is), PV(cc), PV(x0), PV(x1), PV(x2), PV(hh), PV(d0), PV(d1), PV(d2), PV(n0), PV(n1), PV(n2));
                    double w = zv * is;
                    double rp = -((double)n0 * x0 + (double)n1 * x1 + (double)n2 * x2) + sv + hh;
                    double adx = -((double)n0 * d0 + (double)n1 * d1 + (double)n2 * d2);
                    double ds = -rp - adx, dz = -zv + cc + w * adx;
                    rmax = fmax(rmax, fmax(-ds * is, -dz * rcp_nr(zv)));
                    rt1[r] = ds; rt2[r] = dz;
                }
                block_reduce(rmax, 0.0, 0.0, 0.0, 0.0, 1, -1, -1, -1, -1);
                alpha = rv[0] > tau ? tau / rv[0] : 1.0;      // min(1, tau / max ratio); no row limits the step: 1
                if (a.trace && qi == a.trace_agent && tid == 0 && iters < 64) a.trace[iters * 8 + 5] = alpha;
                if (wave == 0) {
                    if (lane < NY) S.y[lane] += alpha * S.dy[lane];
                    compute_x_wave0(S.y, S.x, true);
                }
                __syncthreads();
                iters++;
                phase = ST_PRED;
                stamp(PH_P45);
            }
        }
        if (failed) {
            // warm start did not converge: fall back to the cold start.  Cold start of a handed-over agent (attempt 2) did not converge: the
            // warm start's second opinion -- but only when the cold start gave up ON A FEASIBLE POINT WITH A CLOSED GAP (primal residual at
            // round-off, gap within the relaxed acceptance test's 1e-7): then "infeasible" would be a wrong verdict, whatever made the start
            // fail (seed 9500131: gap 1e-11, residual 1e-15, the step still 4e-7 when K lost definiteness), and the other start converges.
            // An infeasible QP never gets there -- its multipliers run away, also when the iterates stand on a point that violates nothing
            // by more than 1e-9 (the marginal infeasibilities of corridor worlds) --; those agents keep paying ONE start (configs[3]: 16
            // instead of 26 iterations per hand-over).
            if (attempt == 0 || (attempt == 2 && rpmax <= 1e-9 * hmax && gap <= 1e-7 * (1.0 + fabs(obj)))) {
                phase = attempt == 0 ? ST_START_COLD : ST_START_WARM;
                attempt = 1;
                spent += iters;
                iters = 0;
            } else {
                break;
            }
        }
    }
    iters += spent;

    // ------------------------------------------------------------------ output
    // success: float32 rounding of the optimum (src/traj_optimizer.cpp:79-96); failure: the optimiser's
    // previous trajectory is reused (src/traj_planner.cpp:1553-1584)
    float *out = a.traj_next + (size_t)qi * NV;
    float *stale = a.stale + (size_t)qi * NV;
    if (tid < NV) {
        if (status == LSC_STATUS_OK_K) {
            float v = (float)S.x[tid];
            if (dim2 && tid >= 2 * SEGV) v = (float)md.z2d;        // octomap::point3d(x, y, param.world_z_2d), src/traj_optimizer.cpp:87-90
            out[tid] = v; stale[tid] = v;
        } else {
            float v = stale[tid];
            // planar world: a plan is in the plane whatever the optimiser's stale trajectory holds (lsc_set_agents starts its z block
            // at z_2d; this covers a stale plan that came from anywhere else)
            if (dim2 && tid >= 2 * SEGV) { v = (float)md.z2d; stale[tid] = v; }
            out[tid] = v;
        }
    }
    if (a.state_next && tid < 3) {
#pragma clang fp contract(off)
        // MultiSyncSimulator::update for the next tick, fused: ideal state at t = dt on the trajectory just written
        // (getStateFromControlPoints, include/polynomial.hpp:63-97: segment 1, local time 0; float32, unfused)
        const int k = tid;
        float c0, c1, c2;
        if (status == LSC_STATUS_OK_K) {
            c0 = (float)S.x[k * SEGV + NC]; c1 = (float)S.x[k * SEGV + NC + 1]; c2 = (float)S.x[k * SEGV + NC + 2];
            if (dim2 && k == 2) c0 = c1 = c2 = (float)md.z2d;
        } else {
            c0 = stale[k * SEGV + NC]; c1 = stale[k * SEGV + NC + 1]; c2 = stale[k * SEGV + NC + 2];
            if (dim2 && k == 2) c0 = c1 = c2 = (float)md.z2d;
        }
        const float fn = (float)DEG, fn1 = (float)(DEG - 1), finv = a.finv;
        const float v0 = ((c1 - c0) * fn) * finv;
        const float v1 = ((c2 - c1) * fn) * finv;
        const float a0 = ((v1 - v0) * fn1) * finv;
        a.state_next[9 * qi + k] = c0;
        a.state_next[9 * qi + 3 + k] = v0;
        a.state_next[9 * qi + 6 + k] = a0;
    }
    if (tid == 0) {
        if (status == LSC_STATUS_OK_K) a.cost[qi] = obj;
        a.status[qi] = status;
        a.iters[qi] = iters;
        // (atomics without a return value: a read-modify-write in program order put a trip to HBM in front of the end of every workgroup)
        if (a.iters_acc) {
            atomicAdd((unsigned long long *)&a.iters_acc[qi], (unsigned long long)(long long)iters);
            atomicAdd((unsigned long long *)&a.iters_acc[a.N + qi], (unsigned long long)((long long)iters * S.nact));
        }
        if (a.nrows) a.nrows[qi] = S.nact;
        if constexpr (SOLVER == 1) {
            // (only agents whose QP ran here: a goal / corridor error, a capacity overflow or the hand-over of a disturbed swarm to lsc_general_kernel
            //  is neither a finished solve nor a hand-over to the interior point)
            if (a.solver_stats && (status == LSC_STATUS_OK_K || status == LSC_STATUS_INFEASIBLE_K)) {
                // [0] agent-replans the active-set solve finished, [1] those it handed to the interior point, [2] working-set changes, [3] interior-point iterations
                const bool by_gi = run_gi_done;
                // (this agent's own four counters: lsc_solver_stats sums over the agents)
                long long *st = a.solver_stats + 4 * (size_t)qi;
                atomicAdd((unsigned long long *)&st[by_gi ? 0 : 1], 1ull);
                atomicAdd((unsigned long long *)&st[2], (unsigned long long)gi_changes);
                if (!by_gi) atomicAdd((unsigned long long *)&st[3], (unsigned long long)(iters - gi_changes));
            }
        }
        if (a.dbg) { a.dbg[4 * qi] = S.sc[5]; a.dbg[4 * qi + 1] = S.sc[6]; a.dbg[4 * qi + 2] = spent > 0 ? 1000.0 + (double)spent : rv[3]; a.dbg[4 * qi + 3] = obj; }
        if constexpr (PROF) {
            stamp(PH_OUT);
            if (a.prof)
                for (int i = 0; i < PH_COUNT; i++) a.prof[(size_t)qi * PH_COUNT + i] += t_acc[i];
        }
    }
    if constexpr (PROF) { if (tid == NT - 1 && a.prof) a.prof[(size_t)qi * PH_COUNT + PH_RED_GATHER] += t_acc[PH_RED_GATHER]; }
    if constexpr (ALT) return __builtin_amdgcn_readfirstlane(status) == LSC_STATUS_GENERAL_K;
    else return false;
}

template <bool PROF, bool DIM2, int SOLVER = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lsc_plan_kernel(PlanArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // (a timed launch group's clock stamps: lsc_kernels.h, LaunchEvents.  The instrumented kernels stamp nothing: run_plan times a profiled
    //  launch by events)
    const long long t_entry = PROF ? 0 : stamp_clock();
    plan_agent<PROF, false, false, NT, DIM2, const PlanArgs, SOLVER>(a, blockIdx.x, smem_raw, nullptr);
    if constexpr (!PROF) stamp_exit(kernarg_block<PlanArgs>(), t_entry);
}

// ... of a context with dynamic obstacles (lsc_set_obstacles; a.obs): the 3-D latency kernel whose obstacle list is N - 1 agents + K spheres
template <int SOLVER>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lsc_plan_obs_kernel(PlanArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const long long t_entry = stamp_clock();
    plan_agent<false, false, false, NT, false, const PlanArgs, SOLVER, true>(a, blockIdx.x, smem_raw, nullptr);
    stamp_exit(kernarg_block<PlanArgs>(), t_entry);
}

// the same kernel with the alternate-mode hooks (contexts with reset_threshold > 0, BVC or a slack mode).  With a.fold, an agent phase A
// hands over is solved right here, by the same workgroup (lsc_general.hpp: general_fold), instead of by a launch of lsc_general_kernel
// behind this one: on the unflagged path that launch found nothing to do and cost 3-4 us per tick.
template <bool DIM2, int SOLVER = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lsc_plan_alt_kernel(PlanArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const long long t_entry = stamp_clock();
    const bool handed = plan_agent<false, false, true, NT, DIM2, const PlanArgs, SOLVER>(a, blockIdx.x, smem_raw, nullptr);
    if (handed && a.fold) {
#if defined(__HIP_DEVICE_COMPILE__)
        gen::general_fold((KArgs *)__builtin_amdgcn_kernarg_segment_ptr(), blockIdx.x, smem_raw);
#endif
    }
    stamp_exit(kernarg_block<PlanArgs>(), t_entry);    // (behind the folded hand-over as well: the workgroup's one way out)
}

// ... of a context with dynamic obstacles AND the disturbance checks (lsc_set_obstacles_ex): phase A's checks, the fold of the hand-over and
// the reset initial trajectory as above, phase B over N - 1 agents + K spheres as lsc_plan_obs_kernel -- skipped, as above, for a flagged
// swarm, whose rows general_agent<., true> builds (lsc_general.hpp)
template <int SOLVER>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lsc_plan_alt_obs_kernel(PlanArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const long long t_entry = stamp_clock();
    const bool handed = plan_agent<false, false, true, NT, false, const PlanArgs, SOLVER, true>(a, blockIdx.x, smem_raw, nullptr);
    if (handed && a.fold) {
#if defined(__HIP_DEVICE_COMPILE__)
        gen::general_fold<true>((KArgs *)__builtin_amdgcn_kernarg_segment_ptr(), blockIdx.x, smem_raw);
#endif
    }
    stamp_exit(kernarg_block<PlanArgs>(), t_entry);
}

// Throughput build for swarms larger than the chip (more agents in the shard than CUs): 256 lanes = one wave per SIMD, and
// an LDS request of at most half a CU's 160 KB, so that two agents share a CU and one hides the other's latencies (the
// solver is a chain of dependent LDS / cross-lane operations: VALU active 13 % of wave-cycles in the latency build).
template <bool DIM2, int SOLVER = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void lsc_plan_tp_kernel(PlanArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // (the throughput kernels stamp nothing: a timed group that takes them rides on events -- run_plan, lsc_abi.cpp)
    plan_agent<false, false, false, 256, DIM2, const PlanArgs, SOLVER>(a, a.order ? a.order[blockIdx.x] : (int)blockIdx.x, smem_raw, nullptr);
}

// ... its instrumented variant (lsc_phase_profile on a shard larger than the chip: where the throughput build's time goes)
template <int SOLVER = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void lsc_plan_tp_prof_kernel(PlanArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    plan_agent<true, false, false, 256, false, const PlanArgs, SOLVER>(a, a.order ? a.order[blockIdx.x] : (int)blockIdx.x, smem_raw, nullptr);
}

// ... and the throughput build with the alternate-mode hooks
template <bool DIM2, int SOLVER = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void lsc_plan_alt_tp_kernel(PlanArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    plan_agent<false, false, true, 256, DIM2, const PlanArgs, SOLVER>(a, a.order ? a.order[blockIdx.x] : (int)blockIdx.x, smem_raw, nullptr);
}

// Several independent swarms in one launch (blockIdx.y = swarm, PlanBatch in lsc_kernels.h): the mission-list outer loop of the reference
// (src/multi_sync_simulator_node.cpp:43-70) as a batch axis.  A 64-agent swarm is 64 workgroups on a 256-CU chip; four of them in ONE
// dispatch are placed one per CU (four launches on four streams are not: measured 2.1-2.8x against 3.4-3.9x).
// The swarm's argument block is read where it lies in the kernarg segment; the planning code is the same instantiation otherwise.
template <bool ALT, bool DIM2, int SOLVER = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lsc_plan_batch_kernel(PlanBatch)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
#if defined(__HIP_DEVICE_COMPILE__)
    KArgs *ka = (KArgs *)__builtin_amdgcn_kernarg_segment_ptr() + blockIdx.y;
#else
    KArgs *ka = nullptr;                                                             // (host pass of the single-source build)
#endif
    const long long t_entry = stamp_clock();                                         // (every swarm's workgroups stamp the batch's one slot)
    if ((int)blockIdx.x >= ka->count) { stamp_exit(ka, t_entry); return; }           // (swarms of a batch may differ in size)
    plan_agent<false, false, ALT, NT, DIM2, KArgs, SOLVER>(*ka, blockIdx.x, smem_raw, nullptr);
    stamp_exit(ka, t_entry);
}

// Preparation pass of the throughput build:
//  * bounding sphere (centre, radius; float32, radius rounded up) of the agent's predicted control points of all segments
//    (32 lanes per agent) --
//    what every OTHER agent's obstacle-level pre-cull tests against (phase B of plan_agent);
//  * launch order of the shard (only when it takes more than one round of workgroups): the tick ends with the last
//    workgroup, so the agents that were expensive in the previous tick (iterations x rows) go first and the cheap ones
//    fill the gaps (longest-processing-time-first list scheduling; the hardware dispatches workgroups in blockIdx order).
//    Any content of iters / nrows gives a permutation; results do not depend on it.
__global__ __launch_bounds__(256) void lsc_prep_kernel(PlanArgs a)
{
    constexpr int TILE = 2048;
    __shared__ unsigned tile[TILE];
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const long long t_entry = stamp_clock();           // (a timed group's first launch, never its last: the plan kernel follows)
    if (a.obs_bound) {
        // 32 lanes per agent, one predicted control point each (lanes 30, 31 repeat the last one)
        const int qa = q >> 5, pi = (q & 31) < SEGV ? (q & 31) : SEGV - 1;
        const bool live = qa < a.N;
        F3 po[6];
        load_segment(a.state, a.traj_prev, live ? qa : 0, pi / NC, a.planner_seq, (float)a.model->dt, po);
        F3 me = po[0];
#pragma unroll
        for (int i = 1; i < 6; i++) if (pi % NC == i) me = po[i];
        double cx = (double)me.x, cy = (double)me.y, cz = (double)me.z;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) { cx += __shfl_xor(cx, o, 32); cy += __shfl_xor(cy, o, 32); cz += __shfl_xor(cz, o, 32); }
        // any centre will do as long as the radius is taken around the float32 centre that is stored
        const float fx = (float)(cx * (1.0 / 32.0)), fy = (float)(cy * (1.0 / 32.0)), fz = (float)(cz * (1.0 / 32.0));
        const double ex = (double)me.x - (double)fx, ey = (double)me.y - (double)fy, ez = (double)me.z - (double)fz;
        double r2 = ex * ex + ey * ey + ez * ez;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) r2 = fmax(r2, __shfl_xor(r2, o, 32));
        const float rad = (float)(sqrt(r2) * (1.0 + 1e-6) + 1e-6);      // never below the true radius after the float32 rounding
        if (live && (q & 31) == 0) reinterpret_cast<float4 *>(a.obs_bound)[qa] = make_float4(fx, fy, fz, rad);
    }
    // rank of agent qo among the shard's agents by cost, descending (ties: lower index first); 16 lanes per agent, each
    // counting every 16th competitor out of an LDS tile
    const int count = a.count, first = a.first;
    if (!a.order || (int)((blockIdx.x * blockDim.x) >> 4) >= count) { stamp_exit(kernarg_block<PlanArgs>(), t_entry); return; }   // (whole blocks leave: the loop below has barriers)
    const int *iters = a.iters, *nrows = a.nrows;
    auto cost = [&](int p) { return (unsigned)iters[first + p] * (unsigned)(nrows[first + p] + 600); };
    const int qo = q >> 4, part = q & 15;
    const unsigned cq = qo < count ? cost(qo) : 0u;
    int r = 0;
    for (int p0 = 0; p0 < count; p0 += TILE) {
        const int n = count - p0 < TILE ? count - p0 : TILE;
        __syncthreads();
        for (int p = threadIdx.x; p < n; p += blockDim.x) tile[p] = cost(p0 + p);
        __syncthreads();
        for (int p = part; p < n; p += 16) {
            const unsigned cp = tile[p];
            r += (cp > cq) || (cp == cq && p0 + p < qo);
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) r += __shfl_xor(r, o, 16);
    if (qo < count && part == 0) a.order[r] = qo;
    stamp_exit(kernarg_block<PlanArgs>(), t_entry);
}

// Second pass: agents whose rows did not fit the LDS capacity of the first pass are solved again with their rows in
// HBM.  Persistent workgroups (one workspace each) walk the shard; everybody else's result is left untouched.
template <bool DIM2>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lsc_plan_spill_kernel(PlanArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // The common case is "nobody overflowed": leave before anything else happens (the planning code below keeps part of
    // its loop invariants in scratch; a workgroup without work must not pay for setting them up).
    {                                                  // (a timed group's end only: the second pass is never a group's first launch)
        bool work = false;
        for (int al = blockIdx.x; al < a.count; al += gridDim.x) work |= a.status[a.first + al] == LSC_STATUS_CAPACITY_K;
        if (!work) { stamp_end(kernarg_block<PlanArgs>()); return; }
    }
    unsigned char *ws = a.spill_ws + (size_t)blockIdx.x * a.spill_stride;
    for (int al = blockIdx.x; al < a.count; al += gridDim.x) {
        if (a.status[a.first + al] != LSC_STATUS_CAPACITY_K) continue;   // uniform over the workgroup
        __syncthreads();
        plan_agent<false, true, false, NT, DIM2>(a, al, smem_raw, ws);
        __syncthreads();
    }
    stamp_end(kernarg_block<PlanArgs>());
}

// ... of a context with dynamic obstacles: 27 (N - 1 + K) row slots per workspace.  (The same statements as a kernel of its own: the kernel
// above keeps its text -- as a shared body behind a reference to its argument block it spilled two to four more scalar registers.)
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lsc_plan_spill_obs_kernel(PlanArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    bool work = false;
    for (int al = blockIdx.x; al < a.count; al += gridDim.x) work |= a.status[a.first + al] == LSC_STATUS_CAPACITY_K;
    if (!work) { stamp_end(kernarg_block<PlanArgs>()); return; }
    unsigned char *ws = a.spill_ws + (size_t)blockIdx.x * a.spill_stride;
    for (int al = blockIdx.x; al < a.count; al += gridDim.x) {
        if (a.status[a.first + al] != LSC_STATUS_CAPACITY_K) continue;
        __syncthreads();
        plan_agent<false, true, false, NT, false, const PlanArgs, 0, true>(a, al, smem_raw, ws);
        __syncthreads();
    }
    stamp_end(kernarg_block<PlanArgs>());
}

}  // namespace lsc

// ---------------------------------------------------------------------------------------------------
// launch wrappers (called from lsc_abi.cpp)
// ---------------------------------------------------------------------------------------------------
namespace lsc {

// LDS request of the plan kernel for a capacity of `rows` LSC rows (rows are stored compactly: a total, not per bucket)
size_t plan_smem_bytes(int n_terms, int n_entries, int rows, bool tables_in_lds)
{
    size_t b = tables_in_lds ? sizeof(SmemT<false>) : sizeof(SmemT<true>);
    if (tables_in_lds) {
        b += sizeof(uint32_t) * (size_t)((n_terms + 1) & ~1);
        b += sizeof(uint32_t) * (size_t)(2 * n_entries + 2);
    }
    b += sizeof(double) * (size_t)n_entries;      // constant part of the Hessian entries (both layouts since round 5)
    b += (size_t)rows * (5 * sizeof(double) + 3 * sizeof(float) + sizeof(uint32_t));
    return (b + 15) & ~(size_t)15;
}

// bytes of one workgroup's HBM row workspace (second pass): all 27 n_obs row slots (n_obs = N - 1, + the dynamic obstacles)
size_t plan_spill_bytes(int n_obs)
{
    const size_t R = (size_t)NB * (n_obs > 1 ? n_obs : 1);
    return (R * (5 * sizeof(double) + 3 * sizeof(float) + sizeof(uint32_t)) + 255) & ~(size_t)255;
}

// Which build of the planning code a launch takes.  A key packs the family and the compile-time switches of the instantiation.
enum PlanFamily { PLAN_LATENCY, PLAN_THROUGHPUT, PLAN_BATCH, PLAN_SPILL };
constexpr int plan_key(int family, bool alt, bool dim2, int solver, bool prof, bool obs = false) { return obs << 8 | family << 4 | alt << 3 | dim2 << 2 | solver << 1 | (int)prof; }
constexpr int plan_family(int key) { return (key >> 4) & 15; }

// Every instantiation of the plan kernels: a new one is registered by its row here, and nowhere else.
static const KernelVariant plan_variants[] = {
    //                        alt dim2 solver prof
    {plan_key(PLAN_LATENCY,    0, 0, 0, 0), kernel_address(lsc_plan_kernel<false, false>)},
    {plan_key(PLAN_LATENCY,    0, 0, 0, 1), kernel_address(lsc_plan_kernel<true, false>)},
    {plan_key(PLAN_LATENCY,    0, 1, 0, 0), kernel_address(lsc_plan_kernel<false, true>)},
    {plan_key(PLAN_LATENCY,    0, 0, 1, 0), kernel_address(lsc_plan_kernel<false, false, 1>)},
    {plan_key(PLAN_LATENCY,    0, 0, 1, 1), kernel_address(lsc_plan_kernel<true, false, 1>)},
    {plan_key(PLAN_LATENCY,    0, 1, 1, 0), kernel_address(lsc_plan_kernel<false, true, 1>)},
    {plan_key(PLAN_LATENCY,    1, 0, 0, 0), kernel_address(lsc_plan_alt_kernel<false>)},
    {plan_key(PLAN_LATENCY,    1, 1, 0, 0), kernel_address(lsc_plan_alt_kernel<true>)},
    {plan_key(PLAN_LATENCY,    1, 0, 1, 0), kernel_address(lsc_plan_alt_kernel<false, 1>)},
    {plan_key(PLAN_LATENCY,    1, 1, 1, 0), kernel_address(lsc_plan_alt_kernel<true, 1>)},
    {plan_key(PLAN_THROUGHPUT, 0, 0, 0, 0), kernel_address(lsc_plan_tp_kernel<false>)},
    {plan_key(PLAN_THROUGHPUT, 0, 1, 0, 0), kernel_address(lsc_plan_tp_kernel<true>)},
    {plan_key(PLAN_THROUGHPUT, 0, 0, 1, 0), kernel_address(lsc_plan_tp_kernel<false, 1>)},
    {plan_key(PLAN_THROUGHPUT, 0, 0, 0, 1), kernel_address(lsc_plan_tp_prof_kernel<0>)},
    {plan_key(PLAN_THROUGHPUT, 0, 0, 1, 1), kernel_address(lsc_plan_tp_prof_kernel<1>)},
    {plan_key(PLAN_THROUGHPUT, 1, 0, 0, 0), kernel_address(lsc_plan_alt_tp_kernel<false>)},
    {plan_key(PLAN_THROUGHPUT, 1, 1, 0, 0), kernel_address(lsc_plan_alt_tp_kernel<true>)},
    {plan_key(PLAN_THROUGHPUT, 1, 0, 1, 0), kernel_address(lsc_plan_alt_tp_kernel<false, 1>)},
    {plan_key(PLAN_BATCH,      0, 0, 0, 0), kernel_address(lsc_plan_batch_kernel<false, false>)},
    {plan_key(PLAN_BATCH,      0, 1, 0, 0), kernel_address(lsc_plan_batch_kernel<false, true>)},
    {plan_key(PLAN_BATCH,      1, 0, 0, 0), kernel_address(lsc_plan_batch_kernel<true, false>)},
    {plan_key(PLAN_BATCH,      1, 1, 0, 0), kernel_address(lsc_plan_batch_kernel<true, true>)},
    {plan_key(PLAN_BATCH,      0, 0, 1, 0), kernel_address(lsc_plan_batch_kernel<false, false, 1>)},
    {plan_key(PLAN_BATCH,      0, 1, 1, 0), kernel_address(lsc_plan_batch_kernel<false, true, 1>)},
    {plan_key(PLAN_BATCH,      1, 0, 1, 0), kernel_address(lsc_plan_batch_kernel<true, false, 1>)},
    {plan_key(PLAN_BATCH,      1, 1, 1, 0), kernel_address(lsc_plan_batch_kernel<true, true, 1>)},
    {plan_key(PLAN_SPILL,      0, 0, 0, 0), kernel_address(lsc_plan_spill_kernel<false>)},
    {plan_key(PLAN_SPILL,      0, 1, 0, 0), kernel_address(lsc_plan_spill_kernel<true>)},
    //                                     + obs: a context with dynamic obstacles (3-D, no hooks, not instrumented; no planar, batch or throughput rows)
    {plan_key(PLAN_LATENCY,    0, 0, 0, 0, 1), kernel_address(lsc_plan_obs_kernel<0>)},
    {plan_key(PLAN_LATENCY,    0, 0, 1, 0, 1), kernel_address(lsc_plan_obs_kernel<1>)},
    {plan_key(PLAN_SPILL,      0, 0, 0, 0, 1), kernel_address(lsc_plan_spill_obs_kernel)},
    //                                     + obs + alt: ... with the disturbance checks (lsc_set_obstacles_ex on a context with reset_threshold > 0)
    {plan_key(PLAN_LATENCY,    1, 0, 0, 0, 1), kernel_address(lsc_plan_alt_obs_kernel<0>)},
    {plan_key(PLAN_LATENCY,    1, 0, 1, 0, 1), kernel_address(lsc_plan_alt_obs_kernel<1>)},
};
// the corridor kernels: no selection, but the same opt-in
static const KernelVariant sfc_variants[] = {{0, kernel_address(lsc_sfc_kernel)}, {1, kernel_address(lsc_sfc_batch_kernel)}};

// The large-LDS opt-in is a per-device function attribute: lsc_create calls this once per context after hipSetDevice
// (several contexts on several GPUs of one process each get it on their own device).
hipError_t init_device_kernels()
{
    hipError_t e = allow_full_lds(plan_variants);
    if (e == hipSuccess) e = allow_full_lds(sfc_variants);
    if (e == hipSuccess) e = init_device_general_kernel();
    if (e == hipSuccess) e = init_device_goal_kernel();
    return e;
}

// The key of the build a single launch of `a` takes.  What was asked for and what is built differ in three places; a key that is still
// without a row after them (an instrumented planar launch) has no build, and launch_plan refuses it.
static int plan_key_of(const PlanArgs &a)
{
    const bool alt = plan_alt_hooks(a), dim2 = a.dim2 != 0;      // dim2: planar world, the 60-variable instantiations
    bool prof = a.prof != nullptr;
    int solver = a.solver >= 1 ? 1 : 0;                          // 1: the active-set solve first, the interior point as fallback
    // Throughput build (shards larger than the chip; the dense dumps and the trace are the latency build's).  Its instrumented kernel
    // exists for 3-D worlds without the alternate-mode hooks only: every other instrumented launch takes the latency family.
    const bool tp = a.cap_tp > 0 && !a.out_normal && !a.trace && !(prof && (alt || dim2));
    // The planar throughput kernels are built with the interior point alone.
    if (tp && dim2) solver = 0;
    // The instrumented latency kernel has no alternate-mode hooks: with both asked for the hooks win, on the interior point
    // (the instrumented kernels keep their solver otherwise).
    if (!tp && prof && alt && !dim2) { prof = false; solver = 0; }
    // Dynamic obstacles: rows exist for the plain 3-D latency kernels only -- any other key with them has no row, and launch_plan refuses it
    // (lsc_abi.cpp refuses those contexts by name long before).
    return plan_key(tp ? PLAN_THROUGHPUT : PLAN_LATENCY, alt, dim2, solver, prof, a.obs != nullptr);
}

// whether this launch takes the throughput build (and with it lsc_prep_kernel's bounds / order)
static bool uses_throughput_build(const PlanArgs &a) { return plan_family(plan_key_of(a)) == PLAN_THROUGHPUT; }

// ... for the host: a timed group that takes the throughput kernels rides on events (they stamp nothing)
bool plan_kernel_is_throughput(const PlanArgs &a) { return a.count > 0 && uses_throughput_build(a); }

// whether launch_plan takes the kernel that can solve the hand-over itself: only lsc_plan_alt_kernel folds (not the throughput build, not the batch kernel)
bool plan_kernel_folds(const PlanArgs &a) { return plan_alt_hooks(a) && a.count > 0 && !uses_throughput_build(a); }

hipError_t launch_plan(const PlanArgs &a, size_t smem, hipStream_t st, LaunchEvents ev)
{
    if (a.count == 0) return record_unlaunched(ev, st);   // empty shard (more ranks than agents): nothing to plan
    const int key = plan_key_of(a);
    const void *fn = find_variant(plan_variants, key);
    if (!fn) return hipErrorInvalidValue;         // (the instrumented build exists for 3-D worlds only)
    PlanArgs t = a;
    t.fold = (a.fold && plan_kernel_folds(a)) ? 1 : 0;
    if (plan_family(key) == PLAN_THROUGHPUT) {
        // throughput build: smaller capacity (an agent beyond it takes the second pass), two workgroups per CU
        t.cap = a.cap_tp;
        // (with neighbour lists -- a.nv -- both the bounds and the launch order were left by lsc_neigh.hip's kernels in front of this call)
        const bool prep = (t.order || t.obs_bound) && !a.nv;
        if (prep) (void)launch_variant(kernel_address(lsc_prep_kernel), dim3(((t.obs_bound ? 32 * a.N : 16 * a.count) + 255) / 256), dim3(256), 0, st, t, ev.first());
        return launch_variant(fn, dim3(a.count), dim3(256), a.smem_tp, st, t, prep ? ev.last() : ev);
    }
    // Latency build of a LARGE swarm (a shard of at most one agent per CU out of >= 512 agents: the sharded 1024-agent swarm): without the
    // obstacle-level cull every workgroup walks all 5 (N - 1) units through the unit-level cull -- ten passes of loads and two barriers each
    // at N = 1024, 18.6 of an agent's 50.6 us.  The bounding spheres cost one small launch (lsc_prep_kernel, ~4 us) in front of the tick.
    t.order = nullptr;                            // filled by lsc_prep_kernel only
    bool prep = false;
    if (!a.nv) {                                  // (with lists, the bounds were left by lsc_neigh.hip's build kernel: an agent without a list falls back to them)
        prep = t.obs_bound && a.N >= 512 && !a.out_normal;
        if (prep) (void)launch_variant(kernel_address(lsc_prep_kernel), dim3((32 * a.N + 255) / 256), dim3(256), 0, st, t, ev.first());
        else t.obs_bound = nullptr;
    }
    return launch_variant(fn, dim3(a.count), dim3(NT), smem, st, t, prep ? ev.last() : ev);
}

// n independent swarms (same planar / alternate-mode class, latency build, rows in LDS) in one launch
hipError_t launch_plan_batch(const PlanArgs *a, int n, size_t smem, hipStream_t st, LaunchEvents ev)
{
    if (n < 1 || n > PLAN_BATCH_MAX) return hipErrorInvalidValue;
    const bool alt = plan_alt_hooks(a[0]), d2 = a[0].dim2 != 0;
    bool active_set = true;                                      // the active-set build when every swarm asks for it
    for (int i = 0; i < n; i++) {
        if (plan_alt_hooks(a[i]) != alt || (a[i].dim2 != 0) != d2 || a[i].prof || a[i].out_normal || a[i].trace) return hipErrorInvalidValue;
        active_set = active_set && a[i].solver >= 1;
    }
    PlanBatch b;
    const int grid = fill_batch(b, a, n);
    for (int i = 0; i < n; i++) {
        b.a[i].order = nullptr; b.a[i].obs_bound = nullptr;      // (filled by lsc_prep_kernel only: the throughput build is not batched)
        b.a[i].nv = nullptr; b.a[i].neigh = nullptr;
        if (b.a[i].obs) return hipErrorInvalidValue;             // (no batch rows with dynamic obstacles)
    }
    if (grid == 0) return record_unlaunched(ev, st);
    return launch_variant(find_variant(plan_variants, plan_key(PLAN_BATCH, alt, d2, active_set, false)), dim3(grid, n), dim3(NT), smem, st, b, ev);
}

hipError_t launch_plan_spill(const PlanArgs &a, int slots, size_t smem, hipStream_t st, LaunchEvents ev)
{
    if (a.count == 0 || slots < 1 || !a.spill_ws) return record_unlaunched(ev, st);
    const int grid = a.count < slots ? a.count : slots;
    PlanArgs t = a;
    if (!uses_throughput_build(a) && !a.nv) t.obs_bound = nullptr;      // (bounds of this tick exist only behind the throughput launch or the neighbour-list build)
    return launch_variant(find_variant(plan_variants, plan_key(PLAN_SPILL, false, a.dim2 != 0, 0, false, a.obs != nullptr)), dim3(grid), dim3(NT), smem, st, t, ev);
}

// LDS request of the corridor kernels: six face tables; 0 when the tables are too short or outgrow LDS (no launch)
static size_t sfc_smem_bytes(const SfcArgs &a)
{
    const size_t smem = sizeof(double) * 6 * (size_t)a.table_len;
    return (a.table_len < 8 || smem > LDS_MAX_BYTES) ? 0 : smem;
}

hipError_t launch_sfc(const SfcArgs &a, hipStream_t st, LaunchEvents ev)
{
    if (a.count == 0) return record_unlaunched(ev, st);
    const size_t smem = sfc_smem_bytes(a);
    if (!smem) return hipErrorInvalidValue;
    return launch_variant(kernel_address(lsc_sfc_kernel), dim3(a.count), dim3(64), smem, st, a, ev);
}

hipError_t launch_sfc_batch(const SfcArgs *a, int n, hipStream_t st, LaunchEvents ev)
{
    if (n < 1 || n > PLAN_BATCH_MAX) return hipErrorInvalidValue;
    size_t smem = 0;
    for (int i = 0; i < n; i++) {
        const size_t sm = sfc_smem_bytes(a[i]);
        if (!sm) return hipErrorInvalidValue;
        smem = sm > smem ? sm : smem;
    }
    SfcBatch b;
    const int grid = fill_batch(b, a, n);
    if (grid == 0) return record_unlaunched(ev, st);
    return launch_variant(kernel_address(lsc_sfc_batch_kernel), dim3(grid, n), dim3(64), smem, st, b, ev);
}

hipError_t launch_sweep(const SweepArgs &a, hipStream_t st, LaunchEvents ev)
{
    if (a.count == 0) return record_unlaunched(ev, st);
    long total = (long)a.count * (a.N - 1) * M;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (blocks < 1) blocks = 1;
    return launch_variant(a.out_d32 ? kernel_address(lsc_sweep_kernel<true>) : kernel_address(lsc_sweep_kernel<false>), dim3(blocks), dim3(256), 0, st, a, ev);
}

hipError_t launch_propagate(const float *traj, float *state, int N, double dt, hipStream_t st)
{
    int n = N * 3;
    hipLaunchKernelGGL(lsc_propagate_kernel, dim3((n + 127) / 128), dim3(128), 0, st, traj, state, N, (float)pow(dt, -1));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// savePlanningResult's agent-agent accounting (src/multi_sync_simulator.cpp:446-503) on the device.
//   lsc_sample_kernel : position of every agent at the sample times, getPointFromControlPoints (include/polynomial.hpp) with
//                       the Bernstein weights of each time computed by the caller in the reference's own arithmetic
//   lsc_safety_kernel : one workgroup per own agent: downwash-scaled distance to every other agent over the sum of radii
//                       (distBetweenAgents, include/util.hpp:225-229), minimum and FIRST partner of the minimum per sample time
// ---------------------------------------------------------------------------------------------------
__global__ void lsc_sample_kernel(const float *traj, const double *weights, const int *seg, int n_times, int N, float *pos)
{
#pragma clang fp contract(off)
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_times * N) return;
    const int ti = u / N, q = u % N;
    const float *t = traj + (size_t)q * NV + seg[ti] * NC;
    const double *b = weights + ti * NC;
    for (int k = 0; k < 3; k++) {
        double x = 0.0;
        for (int i = 0; i < NC; i++) x += (double)t[k * SEGV + i] * b[i];
        pos[(size_t)u * 3 + k] = (float)x;
    }
}

__global__ __launch_bounds__(256) void lsc_safety_kernel(const float *pos, const double *radius, const double *downwash, int n_times, int N,
                                                           int first, double *out_ratio, int *out_partner)
{
#pragma clang fp contract(off)
    __shared__ double s_r[4];
    __shared__ int s_q[4];
    const int al = blockIdx.x, qi = first + al, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double r_a = radius[qi], dw_a = downwash[qi];
    for (int ti = 0; ti < n_times; ti++) {
        const float *p = pos + (size_t)ti * N * 3;
        const float px = p[3 * qi], py = p[3 * qi + 1], pz = p[3 * qi + 2];
        double best = 1e300;
        int bq = 0x7fffffff;
        for (int qj = tid; qj < N; qj += 256) {
            if (qj == qi) continue;
            const double r_b = radius[qj];
            const double dw = (dw_a * r_a + downwash[qj] * r_b) / (r_a + r_b);
            const float dx = px - p[3 * qj], dy = py - p[3 * qj + 1];
            const float dz = (float)((double)(pz - p[3 * qj + 2]) / dw);
            const float n2 = dx * dx + dy * dy + dz * dz;
            const double ratio = sqrt((double)n2) / (r_a + r_b);
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
            for (int w = 1; w < 4; w++)
                if (s_r[w] < r || (s_r[w] == r && s_q[w] < q)) { r = s_r[w]; q = s_q[w]; }
            out_ratio[(size_t)ti * gridDim.x + al] = r;
            out_partner[(size_t)ti * gridDim.x + al] = q == 0x7fffffff ? -1 : q;
        }
        __syncthreads();
    }
}

hipError_t launch_safety(const float *traj, const double *weights, const int *seg, int n_times, int N, int first, int count,
                         const double *radius, const double *downwash, float *pos, double *out_ratio, int *out_partner, hipStream_t st)
{
    const int n = n_times * N;
    hipLaunchKernelGGL(lsc_sample_kernel, dim3((n + 127) / 128), dim3(128), 0, st, traj, weights, seg, n_times, N, pos);
    if (count > 0)
        hipLaunchKernelGGL(lsc_safety_kernel, dim3(count), dim3(256), 0, st, pos, radius, downwash, n_times, N, first, out_ratio, out_partner);
    return hipGetLastError();
}

hipError_t launch_gjk(const double *pts, int count, double *v, double *dist, hipStream_t st)
{
    hipLaunchKernelGGL(lsc_gjk_kernel, dim3((count + 255) / 256), dim3(256), 0, st, pts, count, v, dist);
    return hipGetLastError();
}

}  // namespace lsc
