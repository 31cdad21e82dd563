// launch_particles.hip — spray particles (device/k_particles.h): three launches per step, the move with the
// fates of every item, the scan over the items with the count table, and the scatter with the append; the
// kernel boundaries are the ordering between them. The move and the scatter run on launch_points' grid
// (launch_common.h).
#include "device/k_particles.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

int64_t particle_items(int64_t capacity) { return (capacity + kParticleItem - 1) / kParticleItem; }

// table (padded to 256 B) | offset int64[items][2] | ballots uint64[items][4][2] | partial uint32[items][2]
size_t particle_scratch_bytes(int64_t capacity)
{
  return 256 + (size_t)particle_items(capacity) *
                   (2 * sizeof(int64_t) + 2 * kParticleWaves * sizeof(unsigned long long) + 2 * sizeof(uint32_t));
}

void particle_scratch(void* scratch, int64_t capacity, ParticleCall& c)
{
  unsigned char* b = static_cast<unsigned char*>(scratch);
  const size_t items = (size_t)particle_items(capacity);
  c.table = reinterpret_cast<int64_t*>(b);
  c.offset = reinterpret_cast<int64_t*>(b + 256);
  c.ballots = reinterpret_cast<unsigned long long*>(c.offset + 2 * items);
  c.partial = reinterpret_cast<uint32_t*>(c.ballots + 2 * kParticleWaves * items);
}

hipError_t launch_particles_step(const ParticleCall& c, const SurfaceParams& p, hipStream_t stream, int cus)
{
  if (c.capacity < 1 || c.capacity > ((int64_t)1 << 28) || !c.table || !c.cur || !c.next || c.landed_capacity < 0 ||
      (c.landed_capacity > 0 && !c.landed_out) || (c.emit && !c.emit_counts) || p.count < 1 ||
      p.count > kMaxSurfaceCascades)
    return hipErrorInvalidValue;
  // an item per workgroup (launch_points, launch_common.h), sized from the capacity: the count stays on the
  // device
  static_assert(kParticleItem == kParticleThreads, "one particle per thread of an item");
  hipError_t e = launch_points(k_particles_move, kParticleThreads, c.capacity, stream, cus, c, p);
  if (e != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_particles_scan, dim3(1), dim3(kParticleScanThreads), 0, stream, c);
  if ((e = hipGetLastError()) != hipSuccess)
    return e;
  return launch_points(k_particles_scatter, kParticleThreads, c.capacity, stream, cus, c);
}

hipError_t launch_particles_reset(int64_t* table, int64_t alive, hipStream_t stream)
{
  hipLaunchKernelGGL(k_particles_reset, dim3(1), dim3(64), 0, stream, table, alive);
  return hipGetLastError();
}

}  // namespace oceanfft
