// launch_foam_deposit.hip — ocean_foam_deposit (device/k_foam_deposit.h): three launches per call, the adds
// into the accumulators, the owners' updates of the foam maps, and the fold of the workgroups' counts into the
// table; the kernel boundaries are the ordering between them. The record count stays on the device, so the
// grids are sized from max_records.
#include "device/k_foam_deposit.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

// table (padded to 512 B) | taps uint32[kFoamDepositMaxGrid][16] | owned uint32[kFoamDepositMaxGrid][16][2]
size_t foam_deposit_scratch_bytes()
{
  return 512 + (size_t)kFoamDepositMaxGrid * kMaxSurfaceCascades * 3 * sizeof(uint32_t);
}

void foam_deposit_scratch(void* scratch, FoamDepositCall& c)
{
  unsigned char* b = static_cast<unsigned char*>(scratch);
  static_assert(kFoamDepositCounts * sizeof(int64_t) <= 512, "the table's pad");
  c.table = reinterpret_cast<int64_t*>(b);
  c.taps = reinterpret_cast<uint32_t*>(b + 512);
  c.owned = c.taps + (size_t)kFoamDepositMaxGrid * kMaxSurfaceCascades;
}

template <bool MERGE>
static hipError_t deposit(FoamDepositCall& c, hipStream_t stream, int cus)
{
  int64_t items = (c.max_records + kFoamDepositItem - 1) / kFoamDepositItem;  // <= 2^20
  if (items > kFoamDepositMaxGrid)
    items = kFoamDepositMaxGrid;
  c.grid_add = persistent_grid(k_foam_deposit_add<MERGE>, kFoamDepositThreads, 0, (int)items, cus);
  c.grid_apply = persistent_grid(k_foam_deposit_apply<MERGE>, kFoamDepositThreads, 0, (int)items, cus);
  hipLaunchKernelGGL(k_foam_deposit_add<MERGE>, dim3((unsigned)c.grid_add), dim3(kFoamDepositThreads), 0, stream, c);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_foam_deposit_apply<MERGE>, dim3((unsigned)c.grid_apply), dim3(kFoamDepositThreads), 0, stream, c);
  return hipGetLastError();
}

hipError_t launch_foam_deposit(FoamDepositCall c, bool merge, hipStream_t stream, int cus)
{
  if (c.max_records < 1 || c.max_records > ((int64_t)1 << 28) || !c.records || !c.table || !c.taps || !c.owned ||
      c.pairs < 1 || c.pairs > kMaxSurfaceCascades || c.n < 16 || c.n > 16384 || (c.n & (c.n - 1)) != 0)
    return hipErrorInvalidValue;
  for (int i = 0; i < c.pairs; i++)
    if (!c.c[i].foam)
      return hipErrorInvalidValue;
  hipError_t e = merge ? deposit<true>(c, stream, cus) : deposit<false>(c, stream, cus);
  if (e != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_foam_deposit_fold, dim3(1), dim3(kFoamDepositFoldThreads), 0, stream, c);
  return hipGetLastError();
}

}  // namespace oceanfft
