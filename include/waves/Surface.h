// waves/Surface.h — the renderer's use of the maps as a compute step.
// WaveRenderer::Render (reference src/Renderer.cpp:53-72) binds the three generators' maps and
// draws the plane mesh with resources/waveShader.glsl, whose vertex stage displaces each vertex by
// the cascades (:101-110) and whose fragment stage derives the slope normal and foam (:127-144).
// SurfaceSampler evaluates that sampling per mesh vertex on the GPU and hands the renderer final
// vertices instead of textures.
#pragma once

#include <cstdint>
#include <vector>

#include "oceanfft.h"
#include "vision/RenderDevice.h"
#include "waves/FFTCalculator.h"
#include "waves/Generator.h"

namespace Waves
{

class SurfaceSampler
{
public:
  explicit SurfaceSampler(Vision::RenderDevice* device) : renderDevice(device) {}
  ~SurfaceSampler();
  SurfaceSampler(const SurfaceSampler&) = delete;
  SurfaceSampler& operator=(const SurfaceSampler&) = delete;

  // The reference plane mesh (res x res quads, src/Renderer.cpp:18) around the camera
  // (camera = viewInverse[3].xyz, then forward.xz = -viewInverse[0].xz, waveShader.glsl:84-92),
  // sampled on generators[i]'s maps (Renderer.cpp:62-72). Returns a buffer texture of
  // 2*(res+1) x (res+1) RGBA32F texels: per vertex (x, y, z, jacobian), (nx, ny, nz, 0).
  // Enqueued on the device's stream; the texture is owned by the sampler and reused.
  Vision::ID Sample(const std::vector<Generator*>& generators, const float camera[5], int res);

  // The opposite direction (ocean_surface_query, oceanfft.h): the water surface above `points` world
  // positions xzDevice (x, z pairs in device memory), for floating bodies, buoys and shoreline probes.
  // The fixed point p <- p + (q - V(p).xz) runs at most `iterations` (0..64) steps per point and stops
  // once the residual is <= tolerance metres. Returns a buffer texture of 2*points x 1 RGBA32F texels:
  // per point (base x, water height, base z, jacobian), (nx, ny, nz, residual). The iteration does not
  // converge on folded crests; the residual says so, the call does not fail. Enqueued on the device's
  // stream; the texture is owned by the sampler and reused while `points` stays the same.
  Vision::ID Query(const std::vector<Generator*>& generators, const float* xzDevice, int64_t points, int iterations,
                   float tolerance);

  // Sample with the footprint the camera warp gives each vertex (ocean_surface_sample_plane_lod,
  // oceanfft.h): two levels of each generator's mip pyramid, blended, instead of level 0, so far vertices
  // no longer point-sample maps they step across by many texels. Every generator needs
  // Generator::GenerateMips() since its last CalculateOcean. Same texture layout as Sample, with the
  // footprint in metres in the last float of each vertex; its own texture, reused at the same res.
  Vision::ID SampleLod(const std::vector<Generator*>& generators, const float camera[5], int res);

  // How the water moves (ocean_surface_velocity, oceanfft.h): the velocity of the water particles whose
  // rest positions are the `points` base points xzDevice (x, z pairs in device memory; for the water
  // above a world position, the base x and z that Query returns), for drag on hull points, motion
  // vectors and spray. Every generator needs Generator::CalculateRates() since its last CalculateOcean.
  // Returns a buffer texture of 2*points x 1 RGBA32F texels: per point (displaced x, y, z, 0),
  // (velocity x, y, z in m/s, 0). Enqueued on the device's stream; its own texture, reused while
  // `points` stays the same.
  Vision::ID Velocity(const std::vector<Generator*>& generators, const float* xzDevice, int64_t points);

  // Where rays meet the water (ocean_surface_raycast, oceanfft.h): sensor models, picking, impacts.
  // raysDevice: rays x 8 floats in device memory (ox, oy, oz, tmin, dx, dy, dz, tmax). Each ray is clipped
  // to the slab of the generators' bounds (+- pad) and marched in advances of at least `step` (with a finite
  // `slope`, the caller's bound on the surface slope, by its clearance when that is more) for at most
  // maxSteps steps; a sign change is narrowed by `refine` bisections. Every evaluation is Query's fixed
  // point (iterations, tolerance) started from the previous one's answer. Every generator needs
  // Generator::BuildBounds() since its last CalculateOcean. Returns a buffer texture of 4*rays x 1 RGBA32F
  // texels: per ray (hit x, y, z, t), (nx, ny, nz, jacobian), (base x, water height, base z, residual),
  // (status 0 hit / 1 outside the slab / 2 left the range / 3 step limit, started below, steps, gap).
  // Enqueued on the device's stream; its own texture, reused while `rays` stays the same.
  Vision::ID Raycast(const std::vector<Generator*>& generators, const float* raysDevice, int64_t rays, float step,
                     int maxSteps, int refine, int iterations, float tolerance, float slope, float pad);

  // The picture a camera sees (ocean_camera_render, oceanfft.h): per pixel the camera's ray is marched as
  // Raycast marches it and the hit is shaded with the reference's water colour, fog and sky
  // (resources/waveShader.glsl), in one fused pass; there is no rasteriser, and the water reaches the far
  // plane. Every generator needs Generator::BuildBounds() since its last CalculateOcean, and with
  // camera.lod_scale > 0 (the fragment stage then reads the mip level of each pixel's footprint) also
  // Generator::GenerateMips(). Returns the image, width x height RGBA32F texels, row 0 on top;
  // GetRenderAux() is (t, view depth, jacobian, status as Raycast's) per pixel and GetRenderBytes() the
  // image as RGBA8. Enqueued on the device's stream; the three textures are owned by the sampler and reused
  // while the size stays the same.
  Vision::ID Render(const std::vector<Generator*>& generators, const ocean_camera& camera, const ocean_shading& shading,
                    const ocean_march& march, int width, int height);
  Vision::ID GetRenderAux() const { return renderAux; }
  Vision::ID GetRenderBytes() const { return renderBytes; }

  // Render with what makes the sea white (ocean_camera_render_layers, oceanfft.h): the persistent foam shaded
  // under the fog (layers.foam_opacity > 0: every generator needs a Generator::AdvanceFoam() or ResetFoam()
  // first) and spray records drawn over the water with a per-pixel depth test: recordsDevice is a
  // SprayParticles pool's GetRecords() with its GetCountsDevice() and capacity, or a SprayEmitter call's records
  // with a device count (null: all maxRecords); a null recordsDevice draws no spray. The same textures as
  // Render, and GetRenderAux2(): (foam, spray depth, hit count, nearest record index, the last two as uint32
  // bits) per pixel. A call replays bit for bit.
  Vision::ID RenderLayers(const std::vector<Generator*>& generators, const ocean_camera& camera,
                          const ocean_shading& shading, const ocean_march& march, const ocean_camera_layers& layers,
                          int width, int height, const float* recordsDevice = nullptr,
                          const int64_t* countDevice = nullptr, int64_t maxRecords = 0);
  Vision::ID GetRenderAux2() const { return renderAux2; }

  // Sample with the persistent foam (ocean_surface_sample_plane_foam, oceanfft.h): the same mesh and the
  // same texture layout as Sample, with the generators' averaged foam in the last float of each vertex,
  // which Sample leaves 0. Every generator needs a Generator::AdvanceFoam() or ResetFoam() first. Its own
  // texture, reused at the same res.
  Vision::ID SampleFoam(const std::vector<Generator*>& generators, const float camera[5], int res);

  // Foam where spray lands (ocean_foam_deposit, oceanfft.h): every record of an impact list (a
  // SprayParticles::Step's impacts with GetCountsDevice() + 4 and their capacity; a null countDevice: all
  // maxRecords) adds to the generators' foam maps at the four texels SampleFoam would read at its position,
  // settings[i] for generators[i]. Integer sums: the order of the records does not matter and a call replays bit
  // for bit. Every generator needs a Generator::AdvanceFoam() or ResetFoam() first. Enqueued on the device's
  // stream; GetDepositCounts is the call's int64[50] table (n, offered, then taps, texels touched and touched
  // texels that saturated per generator) and synchronises.
  void DepositFoam(const std::vector<Generator*>& generators, const ocean_foam_deposit_settings* settings,
                   const float* recordsDevice, const int64_t* countDevice, int64_t maxRecords);
  void GetDepositCounts(const std::vector<Generator*>& generators, int64_t out[50]) const;

  // What the water is doing at world positions, under the surface too (ocean_water_kinematics, oceanfft.h):
  // keels, mooring lines, ROVs, submerged sensors. xyzDevice: points x 3 floats (x, y, z; y up) in device
  // memory. Query's fixed point finds the water column above or below each point; the velocity and the
  // pressure head are read from the generators' depth layers at the point's depth under the surface, blended
  // linearly between the two nearest layers. Every generator needs the same Generator::SetDepthLayers() list
  // and a Generator::CalculateKinematics() since its last CalculateOcean. Returns a buffer texture of
  // 3*points x 1 RGBA32F texels: per point (base x, water height, base z, residual), (velocity x, y, z in
  // m/s, pressure head in m), (depth under the surface, layer, blend factor, wet 0 / 1). Enqueued on the
  // device's stream; its own texture, reused while `points` stays the same.
  Vision::ID Kinematics(const std::vector<Generator*>& generators, const float* xyzDevice, int64_t points,
                        int iterations, float tolerance);

private:
  void RenderTextures(int width, int height, const char* who);
  Vision::ID renderImage = 0, renderAux = 0, renderBytes = 0, renderAux2 = 0, renderScratch = 0;
  int renderWidth = 0, renderHeight = 0;
  Vision::ID waterPoints = 0;
  int64_t waterPointCount = 0;
  Vision::ID verticesFoam = 0;
  int verticesFoamRes = 0;
  Vision::ID rayHits = 0;
  int64_t rayCount = 0;
  Vision::RenderDevice* renderDevice = nullptr;
  Vision::ID vertices = 0;
  int verticesRes = 0;
  Vision::ID queried = 0;
  int64_t queriedPoints = 0;
  Vision::ID verticesLod = 0;
  int verticesLodRes = 0;
  Vision::ID velocities = 0;
  int64_t velocityPoints = 0;
};

// Floating bodies as sets of hull points (ocean_hulls, oceanfft.h): per step, the bodies' poses in and one
// wrench per body out, in one fused pass over the query, the water velocity, the load model and a sum per
// body whose order is fixed, so a step is replayable bit for bit.
class HullSet
{
public:
  // points: nPoints x 8 host floats (lx, ly, lz, volume, half_height, drag_lin, drag_quad, 0) in the body
  // frame; ranges: bodies x 2 host int32 (first, count) into points, which bodies may share (instances of one
  // hull). Copied to the device; throws std::runtime_error on invalid arguments.
  HullSet(Vision::RenderDevice* device, FFTCalculator* fft, const float* points, int64_t nPoints, const int32_t* ranges,
          int bodies);
  ~HullSet();
  HullSet(const HullSet&) = delete;
  HullSet& operator=(const HullSet&) = delete;

  int GetBodies() const { return ocean_hulls_bodies(hulls); }
  int64_t GetInstancePoints() const { return ocean_hulls_instance_points(hulls); }
  ocean_hulls* GetHandle() const { return hulls; }

  // posesDevice: bodies x 20 floats in device memory (R[9] row-major body->world, centre, velocity, angular
  // velocity, 0, 0). Returns a buffer texture of 2*bodies x 1 RGBA32F texels: per body (Fx, Fy, Fz, submerged
  // volume), (Tx, Ty, Tz about the centre, wet points). waterVelocity needs Generator::CalculateRates() since
  // each generator's last CalculateOcean; without it the water is taken at rest. With pointOutput the
  // per-point rows (base x, water height, base z, residual), (Fx, Fy, Fz, submerged fraction) land in
  // GetPointOutput() (2*instancePoints x 1 texels). Enqueued on the device's stream; both textures are owned
  // by the set and reused.
  Vision::ID Loads(const std::vector<Generator*>& generators, const float* posesDevice, float rhoG, int iterations,
                   float tolerance, bool waterVelocity, bool pointOutput = false);
  Vision::ID GetPointOutput() const { return pointRows; }

  // Hull dynamics (ocean_hulls_set_bodies / ocean_hulls_step, oceanfft.h). props: bodies x 8 host floats
  // (mass, Ix, Iy, Iz, lin_damp, ang_damp, kinematic, 0); may be called again to replace them.
  void SetBodies(const float* props);
  // Steps posesDevice in place by settings.dt in settings.substeps substeps under the wave loads, gravity and
  // the optional external wrenches (wrenchExtDevice: bodies x 8 device floats, force in 0..2 and torque about
  // the centre in 4..6, world frame). Returns the loads texture of Loads(), holding the loads at the start of
  // the last substep; with pointOutput the per-point rows land in GetPointOutput(). Enqueued on the device's
  // stream: no host synchronisation.
  Vision::ID Step(const std::vector<Generator*>& generators, float* posesDevice,
                  const ocean_hull_step_settings& settings, const float* wrenchExtDevice = nullptr,
                  bool pointOutput = false);

private:
  Vision::RenderDevice* renderDevice = nullptr;
  ocean_hulls* hulls = nullptr;
  Vision::ID loads = 0;
  Vision::ID pointRows = 0;
};

// Mooring lines (ocean_moorings, oceanfft.h): chains of lumped nodes between anchors fixed in the world and
// fairleads on the bodies of a HullSet, stepped on the device; per call one wrench per body out, in the layout
// HullSet::Step takes as wrenchExtDevice.
class MooringSet
{
public:
  // lines: nLines x 16 host floats (anchor, fairlead, length, EA, CA, mass_per_m, volume_per_m, drag_lin,
  // drag_quad, 0, 0, 0); attach: nLines x 2 host int32 (body or -1, nodes 2..64). Copied to the device; throws
  // std::runtime_error on invalid arguments.
  MooringSet(Vision::RenderDevice* device, FFTCalculator* fft, const float* lines, const int32_t* attach, int nLines,
             int bodies);
  ~MooringSet();
  MooringSet(const MooringSet&) = delete;
  MooringSet& operator=(const MooringSet&) = delete;

  int GetLines() const { return ocean_moorings_lines(moorings); }
  int64_t GetTotalNodes() const { return ocean_moorings_total_nodes(moorings); }
  ocean_moorings* GetHandle() const { return moorings; }
  // The nodes, totalNodes x 8 device floats (x, y, z, T, vx, vy, vz, flags), for the caller to read and write.
  float* GetNodesDevice() { return ocean_moorings_nodes(moorings); }

  // Every line straight from its anchor to its fairlead, at rest. posesDevice: bodies x 20 device floats (null
  // when no line has a body).
  void Reset(const float* posesDevice);
  // Steps the nodes by settings.dt under the frozen posesDevice. generators: the water of settings.water == 1
  // (each with Generator::SetDepthLayers() and a CalculateKinematics() since its last CalculateOcean); empty
  // for still water. Returns the wrench texture, 2*bodies x 1 RGBA32F texels: per body (Fx, Fy, Fz, lines),
  // (Tx, Ty, Tz about the centre, 0); GetWrenchDevice() is its device pointer for HullSet::Step. With
  // lineOutput the per-line rows (mean fairlead force, fairlead tension), (anchor tension, largest tension,
  // nodes on the bed, wet nodes) land in GetLineOutput() (2*lines x 1 texels). Enqueued on the device's
  // stream: no host synchronisation.
  Vision::ID Step(const std::vector<Generator*>& generators, const ocean_mooring_settings& settings,
                  const float* posesDevice, bool lineOutput = false);
  const float* GetWrenchDevice() const;
  Vision::ID GetLineOutput() const { return lineRows; }

private:
  Vision::RenderDevice* renderDevice = nullptr;
  ocean_moorings* moorings = nullptr;
  int bodyCount = 0;
  Vision::ID wrench = 0;
  Vision::ID lineRows = 0;
};

// Emitters at breaking crests (ocean_spray, oceanfft.h): spray, whitecap sprites, splash sounds. Per call the
// texels of the generators' Jacobian maps under their thresholds, thinned by rate * dt, become one ordered,
// dense list of records with the position and velocity of their water particles; the count stays on the
// device, and a call is replayable bit for bit.
class SprayEmitter
{
public:
  SprayEmitter(Vision::RenderDevice* device, FFTCalculator* fft);
  ~SprayEmitter();
  SprayEmitter(const SprayEmitter&) = delete;
  SprayEmitter& operator=(const SprayEmitter&) = delete;

  ocean_spray* GetHandle() const { return spray; }

  // settings: one per generator (host). tiles: generators x 2 host int32 plane offsets, or null. `step`
  // numbers the call: the same step draws the same emitters. velocity needs Generator::CalculateRates() since
  // each generator's last CalculateOcean; without it the velocities are 0. Returns a buffer texture of
  // 2*capacity x 1 RGBA32F texels: per record (x, y, z, threshold - jacobian), (velocity x, y, z in m/s, id as
  // uint32 bits: generator << 28 | texel); records from GetCounts()[0] on are not written. Enqueued on the
  // device's stream; the texture is owned by the emitter and reused while `capacity` stays the same.
  Vision::ID Emit(const std::vector<Generator*>& generators, const ocean_spray_settings* settings, const int32_t* tiles,
                  float dt, uint32_t step, bool velocity, int64_t capacity);
  // (written, found, found per generator ..) of the last Emit; waits for the device's stream
  void GetCounts(int64_t out[18]) const;
  // The same table in device memory
  const int64_t* GetCountsDevice() const;

private:
  Vision::RenderDevice* renderDevice = nullptr;
  ocean_spray* spray = nullptr;
  Vision::ID records = 0;
  int64_t recordCapacity = 0;
};

// A persistent pool of spray particles (ocean_particles, oceanfft.h): per Step every particle moves under
// gravity and drag toward a wind, the ones that reach the water or their lifetime leave, the survivors are
// compacted in their order and a SprayEmitter call's records are appended. The counts stay on the device, and
// a step is replayable bit for bit.
class SprayParticles
{
public:
  SprayParticles(Vision::RenderDevice* device, FFTCalculator* fft, int64_t capacity);
  ~SprayParticles();
  SprayParticles(const SprayParticles&) = delete;
  SprayParticles& operator=(const SprayParticles&) = delete;

  ocean_particles* GetHandle() const { return particles; }

  // One step on the device's stream. emitter with emitRecords (the texture its last Emit returned): the
  // records to append, or null / 0 for none. landedCapacity > 0: the impacts, (x, water height, z, age),
  // (velocity, id), go to a buffer texture of 2*landedCapacity x 1 RGBA32F texels owned by the pool and
  // reused while landedCapacity stays the same, which is returned; else 0 and the impacts are only counted.
  Vision::ID Step(const std::vector<Generator*>& generators, const ocean_particle_settings& settings, float dt,
                  const SprayEmitter* emitter, Vision::ID emitRecords, int64_t landedCapacity);
  // Replaces the list with `count` device records of 8 floats; Clear empties it
  void Load(const float* recordsDevice, int64_t count);
  void Clear();
  // The current list, GetCounts()[0] records of 8 floats: valid until the next Step or Load
  const float* GetRecords() const;
  // (alive, alive before, survivors, landed found, landed written, expired, appended, dropped); waits for the
  // device's stream
  void GetCounts(int64_t out[8]) const;
  // The same table in device memory
  const int64_t* GetCountsDevice() const;

private:
  Vision::RenderDevice* renderDevice = nullptr;
  ocean_particles* particles = nullptr;
  Vision::ID landed = 0;
  int64_t landedCapacity = 0;
};

}  // namespace Waves
