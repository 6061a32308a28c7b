// lsc_general.hip -- lsc_general_kernel: the alternate planner modes (BVC, slack variables, the disturbance reset) on gfx950.
// The solver itself is in lsc_general.hpp.
#include "lsc_general.hpp"

namespace lsc {

using namespace gen;

// Most launches of this kernel find nobody flagged (it follows the plan kernel whenever the disturbance checks are on):
// that case must cost a launch and nothing else.  The argument block is therefore read in place, through the kernarg
// segment pointer -- naming the by-value parameter would make the compiler copy all of it into scratch in the prologue,
// before the exit test.
__global__ __launch_bounds__(GT) void lsc_general_kernel(PlanArgs)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
#if defined(__HIP_DEVICE_COMPILE__)
    KArgs *ka = (KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
#else
    KArgs *ka = nullptr;                                                             // (host pass of the single-source build)
#endif
    // (a timed launch group's clock stamps, lsc_kernels.h: its end only -- this kernel follows the plan kernel, which carries the begin)
    bool work = false;
    for (int al = blockIdx.x; al < ka->count; al += gridDim.x) work |= ka->status[ka->first + al] == LSC_STATUS_GENERAL_K;
    if (!work) { stamp_end(ka); return; }              // (a workgroup that leaves at once stamps its exit like any other)
    general_entry(ka, smem_raw);
    stamp_end(ka);
}

// ... of a context with dynamic obstacles (lsc_set_obstacles_ex; a.obs): the obstacle list is N - 1 agents + K spheres.  A kernel of its
// own, so that the one above keeps its text.
__global__ __launch_bounds__(GT) void lsc_general_obs_kernel(PlanArgs)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
#if defined(__HIP_DEVICE_COMPILE__)
    KArgs *ka = (KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
#else
    KArgs *ka = nullptr;
#endif
    bool work = false;
    for (int al = blockIdx.x; al < ka->count; al += gridDim.x) work |= ka->status[ka->first + al] == LSC_STATUS_GENERAL_K;
    if (!work) { stamp_end(ka); return; }
    general_entry<true>(ka, smem_raw);
    stamp_end(ka);
}

// The same for a batch of independent swarms (blockIdx.y = swarm; lsc_kernels.h: PlanBatch).
__global__ __launch_bounds__(GT) void lsc_general_batch_kernel(PlanBatch)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
#if defined(__HIP_DEVICE_COMPILE__)
    KArgs *ka = (KArgs *)__builtin_amdgcn_kernarg_segment_ptr() + blockIdx.y;
#else
    KArgs *ka = nullptr;
#endif
    // (a timed launch group's clock stamps, lsc_kernels.h: its end only -- this kernel follows the plan kernel, which carries the begin)
    bool work = false;
    for (int al = blockIdx.x; al < ka->count; al += gridDim.x) work |= ka->status[ka->first + al] == LSC_STATUS_GENERAL_K;
    if (!work) { stamp_end(ka); return; }              // (a workgroup that leaves at once stamps its exit like any other)
    general_entry(ka, smem_raw);
    stamp_end(ka);
}

// (N in the three functions below: agents + dynamic obstacles of the context -- N - 1 obstacles per agent)
size_t general_ws_bytes(int N) { return ws_bytes_of(N); }

// dynamic LDS of the solver: its state + as much of the row workspace as fits (lsc_general_kernel; lsc_plan_alt_kernel when it folds)
size_t general_lds_bytes(int N) { return gs_bytes() + ws_lds_bytes(N); }

// kept obstacles of one agent up to which every row array lies in that LDS (lsc_general_info)
int general_lds_obstacles(int N) { return ws_lds_obstacles(N); }

hipError_t init_device_general_kernel()
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lsc_general_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_BYTES);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lsc_general_obs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_BYTES);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&lsc_general_batch_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_BYTES);
}

// n_dyn: the K of a.obs (a device pointer: the host says what it holds)
hipError_t launch_general(const PlanArgs &a, int slots, hipStream_t st, LaunchEvents ev, int n_dyn)
{
    if (a.count == 0 || slots < 1 || !a.gen_ws) return record_unlaunched(ev, st);
    if ((a.obs != nullptr) != (n_dyn > 0)) return hipErrorInvalidValue;
    const int grid = a.count < slots ? a.count : slots;
    const size_t smem = general_lds_bytes(a.N + n_dyn);
    return launch_variant(a.obs ? kernel_address(lsc_general_obs_kernel) : kernel_address(lsc_general_kernel), dim3(grid), dim3(GT), smem, st, a, ev);
}

// n swarms of the same size class in one launch; every swarm's workgroups use ITS workspace (gen_ws of its own block), so `slots`
// is the smallest slot count among them
hipError_t launch_general_batch(const PlanArgs *a, int n, int slots, hipStream_t st, LaunchEvents ev)
{
    if (n < 1 || n > PLAN_BATCH_MAX || slots < 1) return hipErrorInvalidValue;
    int Nmax = 0;
    for (int i = 0; i < n; i++) {
        if (!a[i].gen_ws || a[i].obs) return hipErrorInvalidValue;      // (no batch kernel with dynamic obstacles)
        Nmax = a[i].N > Nmax ? a[i].N : Nmax;
    }
    PlanBatch b;
    const int most = fill_batch(b, a, n), grid = most < slots ? most : slots;
    if (grid == 0) return record_unlaunched(ev, st);
    const size_t smem = general_lds_bytes(Nmax);
    return launch_variant(kernel_address(lsc_general_batch_kernel), dim3(grid, n), dim3(GT), smem, st, b, ev);
}

}  // namespace lsc
