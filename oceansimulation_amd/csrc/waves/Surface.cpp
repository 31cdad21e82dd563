// Waves::SurfaceSampler over ocean_surface_sample_plane / ocean_surface_query /
// ocean_surface_sample_plane_lod / ocean_surface_velocity / ocean_surface_sample_plane_foam / ocean_foam_deposit /
// ocean_water_kinematics / ocean_camera_render / ocean_camera_render_layers, and Waves::HullSet over ocean_hulls
// (include/oceanfft.h).
#include "waves/Surface.h"

#include <stdexcept>
#include <string>

namespace Waves
{

SurfaceSampler::~SurfaceSampler()
{
  if (vertices)
    renderDevice->DestroyTexture2D(vertices);
  if (queried)
    renderDevice->DestroyTexture2D(queried);
  if (verticesLod)
    renderDevice->DestroyTexture2D(verticesLod);
  if (velocities)
    renderDevice->DestroyTexture2D(velocities);
  if (rayHits)
    renderDevice->DestroyTexture2D(rayHits);
  if (verticesFoam)
    renderDevice->DestroyTexture2D(verticesFoam);
  if (waterPoints)
    renderDevice->DestroyTexture2D(waterPoints);
  for (Vision::ID id : {renderImage, renderAux, renderBytes, renderAux2, renderScratch})
    if (id)
      renderDevice->DestroyTexture2D(id);
}

Vision::ID SurfaceSampler::Sample(const std::vector<Generator*>& generators, const float camera[5], int res)
{
  if (!vertices || verticesRes != res)
  {
    if (vertices)
      renderDevice->DestroyTexture2D(vertices);
    Vision::Texture2DDesc desc;
    desc.Width = 2 * (res + 1);
    desc.Height = res + 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    vertices = renderDevice->CreateTexture2D(desc);
    verticesRes = res;
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_surface_sample_plane(gens.data(), cascades.data(), (int)gens.size(), camera, res,
                                            static_cast<float*>(renderDevice->GetTexturePointer(vertices)));
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::Sample: ") + ocean_last_error());
  return vertices;
}

Vision::ID SurfaceSampler::SampleLod(const std::vector<Generator*>& generators, const float camera[5], int res)
{
  if (!verticesLod || verticesLodRes != res)
  {
    if (verticesLod)
      renderDevice->DestroyTexture2D(verticesLod);
    verticesLod = 0;
    Vision::Texture2DDesc desc;
    desc.Width = 2 * (res + 1);
    desc.Height = res + 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    verticesLod = renderDevice->CreateTexture2D(desc);
    verticesLodRes = res;
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_surface_sample_plane_lod(gens.data(), cascades.data(), (int)gens.size(), camera, res,
                                                static_cast<float*>(renderDevice->GetTexturePointer(verticesLod)));
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::SampleLod: ") + ocean_last_error());
  return verticesLod;
}

Vision::ID SurfaceSampler::Query(const std::vector<Generator*>& generators, const float* xzDevice, int64_t points,
                                 int iterations, float tolerance)
{
  if (points < 1)
    throw std::runtime_error("SurfaceSampler::Query: need at least one point");
  if (!queried || queriedPoints != points)
  {
    if (queried)
      renderDevice->DestroyTexture2D(queried);
    queried = 0;
    Vision::Texture2DDesc desc;
    desc.Width = 2 * (std::size_t)points;
    desc.Height = 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    queried = renderDevice->CreateTexture2D(desc);
    queriedPoints = points;
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_surface_query(gens.data(), cascades.data(), (int)gens.size(), xzDevice, points, iterations,
                                     tolerance, static_cast<float*>(renderDevice->GetTexturePointer(queried)));
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::Query: ") + ocean_last_error());
  return queried;
}

Vision::ID SurfaceSampler::Velocity(const std::vector<Generator*>& generators, const float* xzDevice, int64_t points)
{
  if (points < 1)
    throw std::runtime_error("SurfaceSampler::Velocity: need at least one point");
  if (!velocities || velocityPoints != points)
  {
    if (velocities)
      renderDevice->DestroyTexture2D(velocities);
    velocities = 0;
    Vision::Texture2DDesc desc;
    desc.Width = 2 * (std::size_t)points;
    desc.Height = 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    velocities = renderDevice->CreateTexture2D(desc);
    velocityPoints = points;
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_surface_velocity(gens.data(), cascades.data(), (int)gens.size(), xzDevice, points,
                                        static_cast<float*>(renderDevice->GetTexturePointer(velocities)));
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::Velocity: ") + ocean_last_error());
  return velocities;
}

Vision::ID SurfaceSampler::Raycast(const std::vector<Generator*>& generators, const float* raysDevice, int64_t rays,
                                   float step, int maxSteps, int refine, int iterations, float tolerance, float slope,
                                   float pad)
{
  if (rays < 1)
    throw std::runtime_error("SurfaceSampler::Raycast: need at least one ray");
  if (!rayHits || rayCount != rays)
  {
    if (rayHits)
      renderDevice->DestroyTexture2D(rayHits);
    rayHits = 0;
    Vision::Texture2DDesc desc;
    desc.Width = 4 * (std::size_t)rays;
    desc.Height = 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    rayHits = renderDevice->CreateTexture2D(desc);
    rayCount = rays;
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_surface_raycast(gens.data(), cascades.data(), (int)gens.size(), raysDevice, rays, step, maxSteps,
                                       refine, iterations, tolerance, slope, pad,
                                       static_cast<float*>(renderDevice->GetTexturePointer(rayHits)));
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::Raycast: ") + ocean_last_error());
  return rayHits;
}

Vision::ID SurfaceSampler::SampleFoam(const std::vector<Generator*>& generators, const float camera[5], int res)
{
  if (!verticesFoam || verticesFoamRes != res)
  {
    if (verticesFoam)
      renderDevice->DestroyTexture2D(verticesFoam);
    verticesFoam = 0;
    Vision::Texture2DDesc desc;
    desc.Width = 2 * (res + 1);
    desc.Height = res + 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    verticesFoam = renderDevice->CreateTexture2D(desc);
    verticesFoamRes = res;
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_surface_sample_plane_foam(gens.data(), cascades.data(), (int)gens.size(), camera, res,
                                                 static_cast<float*>(renderDevice->GetTexturePointer(verticesFoam)));
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::SampleFoam: ") + ocean_last_error());
  return verticesFoam;
}

void SurfaceSampler::DepositFoam(const std::vector<Generator*>& generators, const ocean_foam_deposit_settings* settings,
                                 const float* recordsDevice, const int64_t* countDevice, int64_t maxRecords)
{
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_foam_deposit(gens.data(), cascades.data(), (int)gens.size(), settings, recordsDevice, countDevice,
                                    maxRecords);
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::DepositFoam: ") + ocean_last_error());
}

void SurfaceSampler::GetDepositCounts(const std::vector<Generator*>& generators, int64_t out[50]) const
{
  if (generators.empty())
    throw std::runtime_error("SurfaceSampler::GetDepositCounts: no generator");
  if (ocean_foam_deposit_counts(generators[0]->GetHandle(), out) != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::GetDepositCounts: ") + ocean_last_error());
}

Vision::ID SurfaceSampler::Kinematics(const std::vector<Generator*>& generators, const float* xyzDevice,
                                      int64_t points, int iterations, float tolerance)
{
  if (points < 1)
    throw std::runtime_error("SurfaceSampler::Kinematics: need at least one point");
  if (!waterPoints || waterPointCount != points)
  {
    if (waterPoints)
      renderDevice->DestroyTexture2D(waterPoints);
    waterPoints = 0;
    Vision::Texture2DDesc desc;
    desc.Width = 3 * (std::size_t)points;
    desc.Height = 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    waterPoints = renderDevice->CreateTexture2D(desc);
    waterPointCount = points;
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_water_kinematics(gens.data(), cascades.data(), (int)gens.size(), xyzDevice, points, iterations,
                                        tolerance, static_cast<float*>(renderDevice->GetTexturePointer(waterPoints)));
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::Kinematics: ") + ocean_last_error());
  return waterPoints;
}

void SurfaceSampler::RenderTextures(int width, int height, const char* who)
{
  if (width < 1 || height < 1)
    throw std::runtime_error(std::string(who) + ": need at least one pixel");
  if (renderImage && renderWidth == width && renderHeight == height)
    return;
  for (Vision::ID* id : {&renderImage, &renderAux, &renderBytes, &renderAux2, &renderScratch})
  {
    if (*id)
      renderDevice->DestroyTexture2D(*id);
    *id = 0;
  }
  Vision::Texture2DDesc desc;
  desc.Width = (std::size_t)width;
  desc.Height = (std::size_t)height;
  desc.PixelType = Vision::PixelType::RGBA32Float;
  renderImage = renderDevice->CreateTexture2D(desc);
  renderAux = renderDevice->CreateTexture2D(desc);
  desc.PixelType = Vision::PixelType::RGBA8;
  renderBytes = renderDevice->CreateTexture2D(desc);
  renderWidth = width;
  renderHeight = height;
}

Vision::ID SurfaceSampler::Render(const std::vector<Generator*>& generators, const ocean_camera& camera,
                                  const ocean_shading& shading, const ocean_march& march, int width, int height)
{
  RenderTextures(width, height, "SurfaceSampler::Render");
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_camera_render(gens.data(), cascades.data(), (int)gens.size(), &camera, &shading, &march, width,
                                     height, static_cast<float*>(renderDevice->GetTexturePointer(renderImage)),
                                     static_cast<float*>(renderDevice->GetTexturePointer(renderAux)),
                                     static_cast<uint8_t*>(renderDevice->GetTexturePointer(renderBytes)));
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::Render: ") + ocean_last_error());
  return renderImage;
}

Vision::ID SurfaceSampler::RenderLayers(const std::vector<Generator*>& generators, const ocean_camera& camera,
                                        const ocean_shading& shading, const ocean_march& march,
                                        const ocean_camera_layers& layers, int width, int height,
                                        const float* recordsDevice, const int64_t* countDevice, int64_t maxRecords)
{
  RenderTextures(width, height, "SurfaceSampler::RenderLayers");
  Vision::Texture2DDesc desc;
  desc.PixelType = Vision::PixelType::RGBA32Float;
  if (!renderAux2)
  {
    desc.Width = (std::size_t)width;
    desc.Height = (std::size_t)height;
    renderAux2 = renderDevice->CreateTexture2D(desc);
  }
  const bool spray = recordsDevice && maxRecords > 0;
  if (spray && !renderScratch)
  {
    desc.Width = (ocean_camera_layers_scratch_bytes(width, height) + 15) / 16;  // texels of 16 bytes
    desc.Height = 1;
    renderScratch = renderDevice->CreateTexture2D(desc);
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_camera_render_layers(
      gens.data(), cascades.data(), (int)gens.size(), &camera, &shading, &march, &layers, width, height, recordsDevice,
      countDevice, maxRecords, spray ? renderDevice->GetTexturePointer(renderScratch) : nullptr,
      static_cast<float*>(renderDevice->GetTexturePointer(renderImage)),
      static_cast<float*>(renderDevice->GetTexturePointer(renderAux)),
      static_cast<float*>(renderDevice->GetTexturePointer(renderAux2)),
      static_cast<uint8_t*>(renderDevice->GetTexturePointer(renderBytes)));
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SurfaceSampler::RenderLayers: ") + ocean_last_error());
  return renderImage;
}

HullSet::HullSet(Vision::RenderDevice* device, FFTCalculator* fft, const float* points, int64_t nPoints,
                 const int32_t* ranges, int bodies)
    : renderDevice(device)
{
  if (ocean_hulls_create(&hulls, fft ? fft->GetPlan() : nullptr, points, nPoints, ranges, bodies) != OCEAN_OK)
    throw std::runtime_error(std::string("HullSet: ") + ocean_last_error());
  Vision::Texture2DDesc desc;
  desc.Width = 2 * (std::size_t)bodies;
  desc.Height = 1;
  desc.PixelType = Vision::PixelType::RGBA32Float;
  loads = renderDevice->CreateTexture2D(desc);
}

HullSet::~HullSet()
{
  ocean_hulls_destroy(hulls);
  if (loads)
    renderDevice->DestroyTexture2D(loads);
  if (pointRows)
    renderDevice->DestroyTexture2D(pointRows);
}

Vision::ID HullSet::Loads(const std::vector<Generator*>& generators, const float* posesDevice, float rhoG,
                          int iterations, float tolerance, bool waterVelocity, bool pointOutput)
{
  if (pointOutput && !pointRows)
  {
    Vision::Texture2DDesc desc;
    desc.Width = 2 * (std::size_t)GetInstancePoints();
    desc.Height = 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    pointRows = renderDevice->CreateTexture2D(desc);
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_hulls_loads(hulls, gens.data(), cascades.data(), (int)gens.size(), posesDevice, rhoG, iterations,
                                   tolerance, waterVelocity ? 1 : 0,
                                   static_cast<float*>(renderDevice->GetTexturePointer(loads)),
                                   pointOutput ? static_cast<float*>(renderDevice->GetTexturePointer(pointRows)) : nullptr);
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("HullSet::Loads: ") + ocean_last_error());
  return loads;
}

void HullSet::SetBodies(const float* props)
{
  if (ocean_hulls_set_bodies(hulls, props) != OCEAN_OK)
    throw std::runtime_error(std::string("HullSet::SetBodies: ") + ocean_last_error());
}

Vision::ID HullSet::Step(const std::vector<Generator*>& generators, float* posesDevice,
                         const ocean_hull_step_settings& settings, const float* wrenchExtDevice, bool pointOutput)
{
  if (pointOutput && !pointRows)
  {
    Vision::Texture2DDesc desc;
    desc.Width = 2 * (std::size_t)GetInstancePoints();
    desc.Height = 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    pointRows = renderDevice->CreateTexture2D(desc);
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_hulls_step(hulls, gens.data(), cascades.data(), (int)gens.size(), &settings, posesDevice,
                                  wrenchExtDevice, static_cast<float*>(renderDevice->GetTexturePointer(loads)),
                                  pointOutput ? static_cast<float*>(renderDevice->GetTexturePointer(pointRows)) : nullptr);
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("HullSet::Step: ") + ocean_last_error());
  return loads;
}

MooringSet::MooringSet(Vision::RenderDevice* device, FFTCalculator* fft, const float* lines, const int32_t* attach,
                       int nLines, int bodies)
    : renderDevice(device), bodyCount(bodies)
{
  if (ocean_moorings_create(&moorings, fft ? fft->GetPlan() : nullptr, lines, attach, nLines, bodies) != OCEAN_OK)
    throw std::runtime_error(std::string("MooringSet: ") + ocean_last_error());
  if (bodies > 0)
  {
    Vision::Texture2DDesc desc;
    desc.Width = 2 * (std::size_t)bodies;
    desc.Height = 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    wrench = renderDevice->CreateTexture2D(desc);
  }
}

MooringSet::~MooringSet()
{
  ocean_moorings_destroy(moorings);
  if (wrench)
    renderDevice->DestroyTexture2D(wrench);
  if (lineRows)
    renderDevice->DestroyTexture2D(lineRows);
}

void MooringSet::Reset(const float* posesDevice)
{
  if (ocean_moorings_reset(moorings, posesDevice) != OCEAN_OK)
    throw std::runtime_error(std::string("MooringSet::Reset: ") + ocean_last_error());
}

const float* MooringSet::GetWrenchDevice() const
{
  return wrench ? static_cast<const float*>(renderDevice->GetTexturePointer(wrench)) : nullptr;
}

Vision::ID MooringSet::Step(const std::vector<Generator*>& generators, const ocean_mooring_settings& settings,
                            const float* posesDevice, bool lineOutput)
{
  if (lineOutput && !lineRows)
  {
    Vision::Texture2DDesc desc;
    desc.Width = 2 * (std::size_t)GetLines();
    desc.Height = 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    lineRows = renderDevice->CreateTexture2D(desc);
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_moorings_step(moorings, gens.data(), cascades.data(), (int)gens.size(), &settings, posesDevice,
                                     wrench ? static_cast<float*>(renderDevice->GetTexturePointer(wrench)) : nullptr,
                                     lineOutput ? static_cast<float*>(renderDevice->GetTexturePointer(lineRows)) : nullptr);
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("MooringSet::Step: ") + ocean_last_error());
  return wrench;
}

SprayEmitter::SprayEmitter(Vision::RenderDevice* device, FFTCalculator* fft) : renderDevice(device)
{
  if (ocean_spray_create(&spray, fft ? fft->GetPlan() : nullptr) != OCEAN_OK)
    throw std::runtime_error(std::string("SprayEmitter: ") + ocean_last_error());
}

SprayEmitter::~SprayEmitter()
{
  ocean_spray_destroy(spray);
  if (records)
    renderDevice->DestroyTexture2D(records);
}

Vision::ID SprayEmitter::Emit(const std::vector<Generator*>& generators, const ocean_spray_settings* settings,
                              const int32_t* tiles, float dt, uint32_t step, bool velocity, int64_t capacity)
{
  if (capacity < 1)
    throw std::runtime_error("SprayEmitter::Emit: need room for at least one record");
  if (!records || recordCapacity != capacity)
  {
    if (records)
      renderDevice->DestroyTexture2D(records);
    records = 0;
    Vision::Texture2DDesc desc;
    desc.Width = 2 * (std::size_t)capacity;
    desc.Height = 1;
    desc.PixelType = Vision::PixelType::RGBA32Float;
    records = renderDevice->CreateTexture2D(desc);
    recordCapacity = capacity;
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const int rc = ocean_spray_emit(spray, gens.data(), cascades.data(), (int)gens.size(), settings, tiles, dt, step,
                                  velocity ? 1 : 0, capacity,
                                  static_cast<float*>(renderDevice->GetTexturePointer(records)));
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SprayEmitter::Emit: ") + ocean_last_error());
  return records;
}

void SprayEmitter::GetCounts(int64_t out[18]) const
{
  if (ocean_spray_counts(spray, out) != OCEAN_OK)
    throw std::runtime_error(std::string("SprayEmitter::GetCounts: ") + ocean_last_error());
}

const int64_t* SprayEmitter::GetCountsDevice() const
{
  const int64_t* table = ocean_spray_counts_device(spray);
  if (!table)
    throw std::runtime_error(std::string("SprayEmitter::GetCountsDevice: ") + ocean_last_error());
  return table;
}

SprayParticles::SprayParticles(Vision::RenderDevice* device, FFTCalculator* fft, int64_t capacity) : renderDevice(device)
{
  if (ocean_particles_create(&particles, fft ? fft->GetPlan() : nullptr, capacity) != OCEAN_OK)
    throw std::runtime_error(std::string("SprayParticles: ") + ocean_last_error());
}

SprayParticles::~SprayParticles()
{
  ocean_particles_destroy(particles);
  if (landed)
    renderDevice->DestroyTexture2D(landed);
}

Vision::ID SprayParticles::Step(const std::vector<Generator*>& generators, const ocean_particle_settings& settings,
                                float dt, const SprayEmitter* emitter, Vision::ID emitRecords, int64_t capacity)
{
  if (capacity < 0)
    throw std::runtime_error("SprayParticles::Step: negative landed capacity");
  if (capacity != landedCapacity)
  {
    if (landed)
      renderDevice->DestroyTexture2D(landed);
    landed = 0;
    if (capacity > 0)
    {
      Vision::Texture2DDesc desc;
      desc.Width = 2 * (std::size_t)capacity;
      desc.Height = 1;
      desc.PixelType = Vision::PixelType::RGBA32Float;
      landed = renderDevice->CreateTexture2D(desc);
    }
    landedCapacity = capacity;
  }
  std::vector<ocean_generator*> gens;
  std::vector<int> cascades;
  for (auto* g : generators)
  {
    gens.push_back(g->GetHandle());
    cascades.push_back(0);
  }
  const bool append = emitter && emitRecords;
  const int rc = ocean_particles_step(
      particles, gens.data(), cascades.data(), (int)gens.size(), &settings, dt,
      append ? static_cast<const float*>(renderDevice->GetTexturePointer(emitRecords)) : nullptr,
      append ? emitter->GetCountsDevice() : nullptr, capacity,
      landed ? static_cast<float*>(renderDevice->GetTexturePointer(landed)) : nullptr);
  if (rc != OCEAN_OK)
    throw std::runtime_error(std::string("SprayParticles::Step: ") + ocean_last_error());
  return landed;
}

void SprayParticles::Load(const float* recordsDevice, int64_t count)
{
  if (ocean_particles_load(particles, recordsDevice, count) != OCEAN_OK)
    throw std::runtime_error(std::string("SprayParticles::Load: ") + ocean_last_error());
}

void SprayParticles::Clear()
{
  if (ocean_particles_clear(particles) != OCEAN_OK)
    throw std::runtime_error(std::string("SprayParticles::Clear: ") + ocean_last_error());
}

const float* SprayParticles::GetRecords() const
{
  const float* records = ocean_particles_records(particles);
  if (!records)
    throw std::runtime_error(std::string("SprayParticles::GetRecords: ") + ocean_last_error());
  return records;
}

void SprayParticles::GetCounts(int64_t out[8]) const
{
  if (ocean_particles_counts(particles, out) != OCEAN_OK)
    throw std::runtime_error(std::string("SprayParticles::GetCounts: ") + ocean_last_error());
}

const int64_t* SprayParticles::GetCountsDevice() const
{
  const int64_t* table = ocean_particles_counts_device(particles);
  if (!table)
    throw std::runtime_error(std::string("SprayParticles::GetCountsDevice: ") + ocean_last_error());
  return table;
}

}  // namespace Waves
