// waveapp_headless.cpp — the reference application's real workload without a window
// (SURVEY §8f rank 1): WaveApp's scene (reference src/Waves.cpp:14-39) driven through the C++
// drop-in exactly like WaveApp::OnUpdate (src/Waves.cpp:59-106), plus the renderer's sampling of
// the maps (waves/Surface.h) and an on-disk export of the last frame.
//
//   one FFTCalculator(N) shared by 3 Generators, plane sizes 5/17/101 m, boundWavelength = 1,
//   wavelength bounds per generator; per frame:
//     dt = 0 while "Q" is held (--freeze A:B, frames A..B-1)            src/Waves.cpp:86-87
//     CalculateOcean(dt, updateSpectrum) for every generator             src/Waves.cpp:90-91
//     the renderer's vertex displacement / normals / foam on the mesh    src/Renderer.cpp:53-84
//   settings edits (--edit F:G.field=value, applied before frame F) set updateSpectrum and redo the
//   wavelength bookkeeping of DrawUI (src/Waves.cpp:177-207). The reference never clears
//   updateSpectrum (src/Waves.cpp:93-94 is commented out), so h0 is re-seeded every frame; with
//   --reseed on-edit it is re-seeded only on the first frame and after edits (the commented-out
//   intent).
//
// Usage: waveapp_headless [--n 256] [--frames 600] [--dt 0.0166667] [--freeze A:B]...
//                         [--edit F:G.field=value]... [--reseed reference|on-edit]
//                         [--mesh RES (0 = no surface step)] [--probes K] [--velocity] [--mips] [--bodies K]
//                         [--float-bodies] [--rays K] [--image WxH] [--dump DIR]
// Prints one JSON line. --dump DIR writes height_G.npy, disp_G.npy, jac_G.npy (G = 0..2),
// surface.npy ((RES+1)^2 x 8 floats) and scene.json for the last frame.
// --probes K (default 0: nothing changes): after the last frame, the water surface above K points on a
// 30 m circle around the camera (a ring of buoys; SurfaceSampler::Query, 8 iterations, tolerance 0).
// The JSON line gains "probes" and "probe_max_residual"; --dump adds probes.npy (K x 8) and
// probe_xz.npy (K x 2).
// --velocity (default off: nothing changes; honoured with --probes K): after the query, every generator's
// rate maps are calculated (Generator::CalculateRates) and SurfaceSampler::Velocity gives the velocity of the
// water at the probes' base points (the query's base x, z). The JSON line gains "probe_max_speed" (m/s);
// --dump adds probe_velocity.npy (K x 8) and height_rate_G.npy / disp_rate_G.npy.
// --mips (default off: nothing changes): after the last frame, every generator's mip pyramid is built
// (Generator::GenerateMips) and the mesh step runs once more through SurfaceSampler::SampleLod, which
// samples each vertex at the level its spacing asks for. The JSON line gains "mips" (levels per map);
// --dump adds height_G_mipL.npy for L = 1 and the top level, and mesh_lod.npy ((RES+1)^2 x 8).
// --bodies K (default 0: nothing changes): K floating bodies, instances of one 4 x 4 x 4-point box hull
// (2 m x 1 m x 4 m), on a 30 m circle around the camera in fixed tilted poses, moving along the circle at
// 1 m/s. Every frame calculates the generators' rate maps and the loads on all bodies (Waves::HullSet::Loads:
// 8 iterations, tolerance 0, water velocity on). The JSON line gains "bodies" and "body_max_residual"; --dump
// adds hull_points.npy (64 x 8), hull_ranges.npy (K x 2, int32), body_poses.npy (K x 20), body_loads.npy
// (K x 8), body_points.npy (64 K x 8) and height_rate_G.npy / disp_rate_G.npy of the last frame.
// --float-bodies (default off: nothing changes; honoured with --bodies K): the bodies are released. Each gets
// the mass of half its displaced volume of water (so it floats half submerged), the moments of inertia of a
// uniform box, damping 0.5 / s, and is stepped every frame by Waves::HullSet::Step (dt as the frame's, 2
// substeps, gravity (0, -9.8, 0), the loads' settings) in place of the loads call; the loads and point rows
// are those of the last substep. The JSON line gains "body_poses" (K rows of 20, the poses after the last
// frame); --dump writes the poses before the first frame to body_poses.npy and adds body_props.npy (K x 8) and
// body_poses_final.npy (K x 20).
// --rays K (default 0: nothing changes): a lidar ring, K rays from a mast at (0, 10, 0), azimuths evenly
// spaced, 5 degrees below the horizon, tmax 400 m. Every frame builds the generators' bounds
// (Generator::BuildBounds) and casts the ring (SurfaceSampler::Raycast: step 0.25, 256 steps, 10 bisections,
// 4 iterations, tolerance 1e-3, fixed steps, pad 0). The JSON line gains "rays" and "ray_hits"; --dump adds
// rays.npy (K x 8), hits.npy (K x 16) and bounds.npy (3 x 18) of the last frame.
// --image WxH (default off: nothing changes): the picture of the reference's camera (ocean_default_camera,
// shading and march). Every frame builds the generators' bounds (Generator::BuildBounds) and renders the image
// (SurfaceSampler::Render). The JSON line gains "image_hits" (pixels whose ray hit the water); --dump adds
// image.npy (H x W x 4), image_aux.npy (H x W x 4: t, depth, jacobian, status) and image8.npy (H x W x 4, uint8)
// of the last frame.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "waves/FFTCalculator.h"
#include "waves/Generator.h"
#include "waves/Surface.h"

namespace
{

struct Edit
{
  int frame = 0, gen = 0;
  std::string field;
  float value = 0.0f;
};

bool set_field(Waves::GeneratorSettings& s, const std::string& f, float v)
{
  // the fields WaveApp::DrawUI edits (src/Waves.cpp:188-198)
  if (f == "U_10") s.U_10 = v;
  else if (f == "theta_0") s.theta_0 = v;
  else if (f == "g") s.g = v;
  else if (f == "scale") s.scale = v;
  else if (f == "displacement") s.displacement = v;
  else if (f == "swell") s.swell = v;
  else if (f == "spread") s.spread = v;
  else if (f == "h") s.h = v;
  else if (f == "F") s.F = v;
  else if (f == "planeSize") s.planeSize = v;
  else return false;
  return true;
}

// numpy .npy v1.0, little-endian float32 (or another 4-byte or 1-byte type: descr), C order
bool write_npy(const std::string& path, const void* data, const std::vector<size_t>& shape, const char* descr = "<f4")
{
  std::string dims;
  size_t count = 1;
  for (size_t d : shape)
  {
    dims += std::to_string(d) + ",";
    count *= d;
  }
  if (shape.size() > 1)
    dims.pop_back();
  std::string header = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (" + dims + "), }";
  const size_t total = 10 + header.size() + 1;
  header.append((64 - total % 64) % 64, ' ');
  header += '\n';
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f)
    return false;
  const unsigned char magic[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
  const uint16_t hl = (uint16_t)header.size();
  bool ok = std::fwrite(magic, 1, 8, f) == 8 && std::fwrite(&hl, 2, 1, f) == 1 &&
            std::fwrite(header.data(), 1, header.size(), f) == header.size() &&
            std::fwrite(data, descr[2] == '1' ? 1 : sizeof(float), count, f) == count;
  return std::fclose(f) == 0 && ok;
}

void usage()
{
  std::fprintf(stderr, "usage: waveapp_headless [--n N] [--frames K] [--dt S] [--freeze A:B]... "
                       "[--edit F:G.field=value]... [--reseed reference|on-edit] [--mesh RES] [--probes K] "
                       "[--velocity] [--mips] [--bodies K] [--float-bodies] [--rays K] [--image WxH] [--dump DIR]\n");
}

}  // namespace

int main(int argc, char** argv)
{
  int n = 256, frames = 600, mesh = 1024, probes = 0, bodies = 0, rays = 0, imageW = 0, imageH = 0;
  float dt = 1.0f / 60.0f;
  bool reseed_every_frame = true, mips = false, velocity = false, floatBodies = false;
  std::string dump;
  std::vector<std::pair<int, int>> freezes;
  std::vector<Edit> edits;
  for (int i = 1; i < argc; i++)
  {
    const std::string a = argv[i];
    if (a == "--mips" || a == "--velocity" || a == "--float-bodies")  // the switches without a value
    {
      (a == "--mips" ? mips : a == "--velocity" ? velocity : floatBodies) = true;
      continue;
    }
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    if (!v)
    {
      usage();
      return 2;
    }
    if (a == "--n") n = std::atoi(v);
    else if (a == "--frames") frames = std::atoi(v);
    else if (a == "--dt") dt = std::strtof(v, nullptr);
    else if (a == "--mesh") mesh = std::atoi(v);
    else if (a == "--probes") probes = std::atoi(v);
    else if (a == "--bodies") bodies = std::atoi(v);
    else if (a == "--rays") rays = std::atoi(v);
    else if (a == "--image")
    {
      if (std::sscanf(v, "%dx%d", &imageW, &imageH) != 2 || imageW < 1 || imageH < 1)
      {
        usage();
        return 2;
      }
    }
    else if (a == "--dump") dump = v;
    else if (a == "--reseed") reseed_every_frame = std::string(v) != "on-edit";
    else if (a == "--freeze")
    {
      int x = 0, y = 0;
      if (std::sscanf(v, "%d:%d", &x, &y) != 2)
      {
        usage();
        return 2;
      }
      freezes.push_back({x, y});
    }
    else if (a == "--edit")
    {
      Edit e;
      char field[64] = {0};
      if (std::sscanf(v, "%d:%d.%63[^=]=%f", &e.frame, &e.gen, field, &e.value) != 4 || e.gen < 0 || e.gen > 2)
      {
        usage();
        return 2;
      }
      e.field = field;
      edits.push_back(e);
    }
    else
    {
      usage();
      return 2;
    }
    i++;
  }
  if (probes < 0 || bodies < 0 || rays < 0)
  {
    usage();
    return 2;
  }

  try
  {
    Vision::RenderDevice device;
    Waves::FFTCalculator fft(&device, (std::size_t)n);
    std::vector<Waves::Generator*> generators;
    static const float primeFactors[] = {5.0f, 17.0f, 101.0f};  // src/Waves.cpp:27
    for (int i = 0; i < 3; i++)
    {
      auto* g = new Waves::Generator(&device, &fft);
      Waves::GeneratorSettings& s = g->GetOceanSettings();
      s.planeSize = primeFactors[i];
      s.boundWavelength = 1;
      s.wavelengthMax = s.planeSize / 2.0;
      s.wavelengthMin = (i == 0) ? 0.0 : primeFactors[i - 1] / 2.0;
      generators.push_back(g);
    }
    Waves::SurfaceSampler sampler(&device);
    const float camera[5] = {0.0f, 5.0f, 0.0f, -0.70711f, 0.70711f};  // src/Renderer.cpp:15-16
    bool updateSpectrum = true;  // src/Waves.h:31
    Vision::ID surface = 0;

    // the floating bodies: one box hull, `bodies` poses on the ring
    const float rhoG = 9810.0f;
    std::vector<float> hullPoints, bodyPoses;
    std::vector<int32_t> hullRanges;
    Waves::HullSet* hulls = nullptr;
    float* posesDevice = nullptr;
    Vision::ID bodyLoads = 0;
    std::vector<float> bodyProps, bodyPosesFinal;
    ocean_hull_step_settings bodyStep;
    ocean_default_hull_step_settings(&bodyStep);
    bodyStep.substeps = 2;
    bodyStep.rho_g = rhoG;
    bodyStep.water_velocity = 1;
    floatBodies = floatBodies && bodies > 0;
    if (bodies > 0)
    {
      for (int k = 0; k < 4; k++)      // z
        for (int j = 0; j < 4; j++)    // y
          for (int i = 0; i < 4; i++)  // x fastest
            for (float f : {(i + 0.5f) * 0.5f - 1.0f, (j + 0.5f) * 0.25f - 0.5f, (k + 0.5f) * 1.0f - 2.0f,
                            0.5f * 0.25f * 1.0f, 0.125f, 40.0f, 15.0f, 0.0f})
              hullPoints.push_back(f);
      for (int b = 0; b < bodies; b++)
      {
        const double a = 2.0 * 3.14159265358979323846 * b / bodies;
        const double roll = 0.2 * std::cos(2.0 * a), pitch = 0.15 * std::sin(3.0 * a);  // about z, then about x
        const double cr = std::cos(roll), sr = std::sin(roll), cp = std::cos(pitch), sp = std::sin(pitch);
        // Rx(pitch) * Rz(roll), row-major
        const double R[9] = {cr, -sr, 0.0, cp * sr, cp * cr, -sp, sp * sr, sp * cr, cp};
        for (double r : R)
          bodyPoses.push_back((float)r);
        for (double c : {camera[0] + 30.0 * std::cos(a), 0.1 * std::cos(5.0 * a) - 0.1, camera[2] + 30.0 * std::sin(a),
                         -std::sin(a), 0.0, std::cos(a),  // 1 m/s along the ring
                         0.0, 0.2, 0.0, 0.0, 0.0})        // yawing at 0.2 rad/s
          bodyPoses.push_back((float)c);
        hullRanges.push_back(0);
        hullRanges.push_back(64);
      }
      hulls = new Waves::HullSet(&device, &fft, hullPoints.data(), 64, hullRanges.data(), bodies);
      if (floatBodies)
      {
        // half the displaced volume of the 2 x 1 x 4 m box in water of rhoG / 9.8 kg/m^3; a uniform box's moments
        const float mass = 0.5f * 8.0f * (rhoG / 9.8f);
        for (int b = 0; b < bodies; b++)
          for (float f : {mass, mass * (1.0f + 16.0f) / 12.0f, mass * (4.0f + 16.0f) / 12.0f, mass * (4.0f + 1.0f) / 12.0f,
                          0.5f, 0.5f, 0.0f, 0.0f})
            bodyProps.push_back(f);
        hulls->SetBodies(bodyProps.data());
      }
      if (hipMalloc(reinterpret_cast<void**>(&posesDevice), bodyPoses.size() * sizeof(float)) != hipSuccess ||
          hipMemcpy(posesDevice, bodyPoses.data(), bodyPoses.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      {
        std::fprintf(stderr, "waveapp_headless: cannot upload the body poses\n");
        return 1;
      }
    }

    // the lidar ring
    std::vector<float> rayData;
    float* raysDevice = nullptr;
    Vision::ID rayHits = 0;
    if (rays > 0)
    {
      const double dep = 5.0 * 3.14159265358979323846 / 180.0;
      for (int k = 0; k < rays; k++)
      {
        const double a = 2.0 * 3.14159265358979323846 * k / rays;
        for (double c : {0.0, 10.0, 0.0, 0.0, std::cos(dep) * std::cos(a), -std::sin(dep), std::cos(dep) * std::sin(a), 400.0})
          rayData.push_back((float)c);
      }
      if (hipMalloc(reinterpret_cast<void**>(&raysDevice), rayData.size() * sizeof(float)) != hipSuccess ||
          hipMemcpy(raysDevice, rayData.data(), rayData.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      {
        std::fprintf(stderr, "waveapp_headless: cannot upload the rays\n");
        return 1;
      }
    }

    // the reference's camera
    ocean_camera imageCamera;
    ocean_shading imageShading;
    ocean_march imageMarch;
    ocean_default_camera(&imageCamera);
    ocean_default_shading(&imageShading);
    ocean_default_march(&imageMarch);
    Vision::ID image = 0;

    device.BeginCommandBuffer();
    device.SubmitCommandBuffer();
    const auto t0 = std::chrono::steady_clock::now();
    int frozen = 0, reseeds = 0;
    for (int f = 0; f < frames; f++)
    {
      bool edited = false;
      for (const Edit& e : edits)
        if (e.frame == f)
        {
          if (!set_field(generators[e.gen]->GetOceanSettings(), e.field, e.value))
          {
            std::fprintf(stderr, "unknown field %s\n", e.field.c_str());
            return 2;
          }
          edited = true;
        }
      if (edited)
      {
        updateSpectrum = true;
        for (int i = 0; i < 3; i++)  // src/Waves.cpp:199-208
        {
          Waves::GeneratorSettings& s = generators[i]->GetOceanSettings();
          s.wavelengthMax = s.planeSize / 2.0;
          s.wavelengthMin = (i == 0) ? 0.0 : generators[i - 1]->GetOceanSettings().planeSize / 2.0;
        }
      }
      float step = dt;
      for (auto& fr : freezes)
        if (f >= fr.first && f < fr.second)
          step = 0.0f;  // "Q" held: src/Waves.cpp:86-87
      frozen += step == 0.0f;
      device.BeginCommandBuffer();
      for (auto* g : generators)
        g->CalculateOcean(step, updateSpectrum);
      reseeds += updateSpectrum;
      if (!reseed_every_frame)
        updateSpectrum = false;
      if (mesh > 0)
        surface = sampler.Sample(generators, camera, mesh);
      if (bodies > 0)
      {
        for (auto* g : generators)
          g->CalculateRates();
        if (floatBodies)
        {
          if (step > 0.0f)  // a frozen frame moves nothing
          {
            bodyStep.dt = step;
            bodyLoads = hulls->Step(generators, posesDevice, bodyStep, nullptr, true);
          }
        }
        else
          bodyLoads = hulls->Loads(generators, posesDevice, rhoG, 8, 0.0f, true, true);
      }
      if (rays > 0)
      {
        for (auto* g : generators)
          g->BuildBounds();
        rayHits = sampler.Raycast(generators, raysDevice, rays, 0.25f, 256, 10, 4, 1e-3f, INFINITY, 0.0f);
      }
      if (imageW > 0)
      {
        if (rays <= 0)
          for (auto* g : generators)
            g->BuildBounds();
        image = sampler.Render(generators, imageCamera, imageShading, imageMarch, imageW, imageH);
      }
      device.SubmitCommandBuffer();
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    std::vector<float> bodyLoadsHost, bodyPointsHost;
    float bodyMaxResidual = 0.0f;
    if (bodies > 0 && frames > 0 && bodyLoads)
    {
      if (floatBodies)
      {
        bodyPosesFinal.resize(bodyPoses.size());  // the last frame's submit has waited for the stream
        if (hipMemcpy(bodyPosesFinal.data(), posesDevice, bodyPoses.size() * sizeof(float), hipMemcpyDeviceToHost) !=
            hipSuccess)
        {
          std::fprintf(stderr, "waveapp_headless: cannot read the body poses\n");
          return 1;
        }
      }
      bodyLoadsHost.resize((size_t)bodies * 8);
      bodyPointsHost.resize((size_t)bodies * 64 * 8);
      device.GetTexture2DDataRaw(bodyLoads, bodyLoadsHost.data());
      device.GetTexture2DDataRaw(hulls->GetPointOutput(), bodyPointsHost.data());
      for (size_t k = 0; k < (size_t)bodies * 64; k++)
        bodyMaxResidual = std::max(bodyMaxResidual, bodyPointsHost[8 * k + 3]);
    }

    std::vector<float> rayHitsHost, boundsHost;
    int rayHitCount = 0;
    if (rays > 0 && frames > 0)
    {
      rayHitsHost.resize((size_t)rays * 16);
      boundsHost.resize(3 * 18);
      device.GetTexture2DDataRaw(rayHits, rayHitsHost.data());
      for (int i = 0; i < 3; i++)
        generators[i]->GetBounds(&boundsHost[18 * (size_t)i]);
      for (int k = 0; k < rays; k++)
        rayHitCount += rayHitsHost[16 * (size_t)k + 12] == 0.0f;
    }

    std::vector<float> imageHost, imageAuxHost;
    std::vector<uint8_t> imageBytesHost;
    int imageHits = 0;
    if (imageW > 0 && frames > 0)
    {
      const size_t px = (size_t)imageW * imageH;
      imageHost.resize(px * 4);
      imageAuxHost.resize(px * 4);
      imageBytesHost.resize(px * 4);
      device.GetTexture2DDataRaw(image, imageHost.data());
      device.GetTexture2DDataRaw(sampler.GetRenderAux(), imageAuxHost.data());
      device.GetTexture2DDataRaw(sampler.GetRenderBytes(), imageBytesHost.data());
      for (size_t k = 0; k < px; k++)
        imageHits += imageAuxHost[4 * k + 3] == 0.0f;
    }

    // the ring of buoys: which water is above each of them now (not part of the timed frames)
    std::vector<float> probeXZ, probeOut;
    std::vector<float> probeVelocity;
    float probeMaxResidual = 0.0f, probeMaxSpeed = 0.0f;
    velocity = velocity && probes > 0;
    if (probes > 0)
    {
      probeXZ.resize((size_t)probes * 2);
      probeOut.resize((size_t)probes * 8);
      for (int k = 0; k < probes; k++)
      {
        const double a = 2.0 * 3.14159265358979323846 * k / probes;
        probeXZ[2 * k] = (float)(camera[0] + 30.0 * std::cos(a));
        probeXZ[2 * k + 1] = (float)(camera[2] + 30.0 * std::sin(a));
      }
      float* xzDevice = nullptr;
      if (hipMalloc(reinterpret_cast<void**>(&xzDevice), probeXZ.size() * sizeof(float)) != hipSuccess ||
          hipMemcpy(xzDevice, probeXZ.data(), probeXZ.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      {
        std::fprintf(stderr, "waveapp_headless: cannot upload the probe positions\n");
        return 1;
      }
      device.BeginCommandBuffer();
      const Vision::ID q = sampler.Query(generators, xzDevice, probes, 8, 0.0f);
      device.SubmitCommandBuffer();
      device.GetTexture2DDataRaw(q, probeOut.data());
      for (int k = 0; k < probes; k++)
        probeMaxResidual = std::max(probeMaxResidual, probeOut[8 * k + 7]);
      if (velocity)
      {
        // how that water moves: the rates of the last frame, sampled at the base points the query found
        std::vector<float> base((size_t)probes * 2);
        for (int k = 0; k < probes; k++)
        {
          base[2 * k] = probeOut[8 * k];
          base[2 * k + 1] = probeOut[8 * k + 2];
        }
        if (hipMemcpy(xzDevice, base.data(), base.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        {
          std::fprintf(stderr, "waveapp_headless: cannot upload the probes' base points\n");
          return 1;
        }
        probeVelocity.resize((size_t)probes * 8);
        device.BeginCommandBuffer();
        for (auto* g : generators)
          g->CalculateRates();
        const Vision::ID v = sampler.Velocity(generators, xzDevice, probes);
        device.SubmitCommandBuffer();
        device.GetTexture2DDataRaw(v, probeVelocity.data());
        for (int k = 0; k < probes; k++)
        {
          const float* u = &probeVelocity[8 * k + 4];
          probeMaxSpeed = std::max(probeMaxSpeed, std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]));
        }
      }
      (void)hipFree(xzDevice);
    }

    // the pyramids of the last frame's maps and the mesh sampled through them (not part of the timed frames)
    int mipLevels = 0;
    Vision::ID surfaceLod = 0;
    if (mips)
    {
      device.BeginCommandBuffer();
      for (auto* g : generators)
        g->GenerateMips();
      if (mesh > 0)
        surfaceLod = sampler.SampleLod(generators, camera, mesh);
      device.SubmitCommandBuffer();
      mipLevels = generators[0]->GetMipLevels();
    }

    if (!dump.empty())
    {
      const size_t texels = (size_t)n * n;
      std::vector<float> buf(texels * 4);
      for (int i = 0; i < 3; i++)
      {
        const std::string s = std::to_string(i);
        device.GetTexture2DDataRaw(generators[i]->GetHeightMap(), buf.data());
        bool ok = write_npy(dump + "/height_" + s + ".npy", buf.data(), {(size_t)n, (size_t)n, 4});
        device.GetTexture2DDataRaw(generators[i]->GetDisplacementMap(), buf.data());
        ok = ok && write_npy(dump + "/disp_" + s + ".npy", buf.data(), {(size_t)n, (size_t)n, 4});
        device.GetTexture2DDataRaw(generators[i]->GetJacobianMap(), buf.data());
        ok = ok && write_npy(dump + "/jac_" + s + ".npy", buf.data(), {(size_t)n, (size_t)n});
        if (!ok)
        {
          std::fprintf(stderr, "cannot write %s\n", dump.c_str());
          return 1;
        }
      }
      if (mesh > 0)
      {
        const size_t pts = (size_t)(mesh + 1) * (mesh + 1);
        std::vector<float> v(pts * 8);
        device.GetTexture2DDataRaw(surface, v.data());
        write_npy(dump + "/surface.npy", v.data(), {pts, 8});
      }
      if (mips)
      {
        bool ok = true;
        for (int i = 0; i < 3; i++)
          for (int level : {1, mipLevels - 1})
          {
            const size_t side = (size_t)n >> level;
            std::vector<float> m(side * side * 4);
            device.GetTexture2DDataRaw(generators[i]->GetHeightMip(level), m.data());
            ok = ok && write_npy(dump + "/height_" + std::to_string(i) + "_mip" + std::to_string(level) + ".npy",
                                 m.data(), {side, side, 4});
          }
        if (mesh > 0)
        {
          const size_t pts = (size_t)(mesh + 1) * (mesh + 1);
          std::vector<float> v(pts * 8);
          device.GetTexture2DDataRaw(surfaceLod, v.data());
          ok = ok && write_npy(dump + "/mesh_lod.npy", v.data(), {pts, 8});
        }
        if (!ok)
        {
          std::fprintf(stderr, "cannot write %s\n", dump.c_str());
          return 1;
        }
      }
      if (velocity || !bodyLoadsHost.empty())
      {
        bool ok = !velocity || write_npy(dump + "/probe_velocity.npy", probeVelocity.data(), {(size_t)probes, 8});
        for (int i = 0; i < 3; i++)
        {
          const std::string s = std::to_string(i);
          device.GetTexture2DDataRaw(generators[i]->GetHeightRateMap(), buf.data());
          ok = ok && write_npy(dump + "/height_rate_" + s + ".npy", buf.data(), {(size_t)n, (size_t)n, 4});
          device.GetTexture2DDataRaw(generators[i]->GetDisplacementRateMap(), buf.data());
          ok = ok && write_npy(dump + "/disp_rate_" + s + ".npy", buf.data(), {(size_t)n, (size_t)n, 4});
        }
        if (!ok)
        {
          std::fprintf(stderr, "cannot write %s\n", dump.c_str());
          return 1;
        }
      }
      if (!bodyLoadsHost.empty() &&
          !(write_npy(dump + "/hull_points.npy", hullPoints.data(), {64, 8}) &&
            write_npy(dump + "/hull_ranges.npy", hullRanges.data(), {(size_t)bodies, 2}, "<i4") &&
            write_npy(dump + "/body_poses.npy", bodyPoses.data(), {(size_t)bodies, 20}) &&
            write_npy(dump + "/body_loads.npy", bodyLoadsHost.data(), {(size_t)bodies, 8}) &&
            write_npy(dump + "/body_points.npy", bodyPointsHost.data(), {(size_t)bodies * 64, 8}) &&
            (bodyPosesFinal.empty() ||
             (write_npy(dump + "/body_props.npy", bodyProps.data(), {(size_t)bodies, 8}) &&
              write_npy(dump + "/body_poses_final.npy", bodyPosesFinal.data(), {(size_t)bodies, 20})))))
      {
        std::fprintf(stderr, "cannot write %s\n", dump.c_str());
        return 1;
      }
      if (!rayHitsHost.empty() && !(write_npy(dump + "/rays.npy", rayData.data(), {(size_t)rays, 8}) &&
                                    write_npy(dump + "/hits.npy", rayHitsHost.data(), {(size_t)rays, 16}) &&
                                    write_npy(dump + "/bounds.npy", boundsHost.data(), {3, 18})))
      {
        std::fprintf(stderr, "cannot write %s\n", dump.c_str());
        return 1;
      }
      if (!imageHost.empty() &&
          !(write_npy(dump + "/image.npy", imageHost.data(), {(size_t)imageH, (size_t)imageW, 4}) &&
            write_npy(dump + "/image_aux.npy", imageAuxHost.data(), {(size_t)imageH, (size_t)imageW, 4}) &&
            write_npy(dump + "/image8.npy", imageBytesHost.data(), {(size_t)imageH, (size_t)imageW, 4}, "|u1")))
      {
        std::fprintf(stderr, "cannot write %s\n", dump.c_str());
        return 1;
      }
      if (probes > 0 && !(write_npy(dump + "/probes.npy", probeOut.data(), {(size_t)probes, 8}) &&
                          write_npy(dump + "/probe_xz.npy", probeXZ.data(), {(size_t)probes, 2})))
      {
        std::fprintf(stderr, "cannot write %s\n", dump.c_str());
        return 1;
      }
      FILE* js = std::fopen((dump + "/scene.json").c_str(), "w");
      if (js)
      {
        std::fprintf(js, "{\"n\": %d, \"frames\": %d, \"mesh\": %d, \"camera\": [%g, %g, %g, %g, %g], \"cascades\": [", n,
                     frames, mesh, camera[0], camera[1], camera[2], camera[3], camera[4]);
        for (int i = 0; i < 3; i++)
        {
          const Waves::GeneratorSettings& s = generators[i]->GetOceanSettings();
          std::fprintf(js, "%s{\"planeSize\": %.9g, \"time\": %.9g, \"U_10\": %.9g, \"displacement\": %.9g}",
                       i ? ", " : "", s.planeSize, s.time, s.U_10, s.displacement);
        }
        std::fprintf(js, "]");
        if (bodies > 0)
        {
          std::fprintf(js, ", \"bodies\": {\"count\": %d, \"rho_g\": %.9g, \"iterations\": 8, \"tolerance\": 0", bodies, rhoG);
          if (floatBodies)
            std::fprintf(js, ", \"dt\": %.9g, \"substeps\": %d, \"gravity\": [%.9g, %.9g, %.9g]", dt, bodyStep.substeps,
                         bodyStep.gravity[0], bodyStep.gravity[1], bodyStep.gravity[2]);
          std::fprintf(js, "}");
        }
        std::fprintf(js, "}\n");
        std::fclose(js);
      }
    }
    std::string probeJson;
    if (probes > 0)
    {
      char b[96];
      std::snprintf(b, sizeof b, ", \"probes\": %d, \"probe_max_residual\": %.9g", probes, probeMaxResidual);
      probeJson = b;
    }
    if (velocity)
    {
      char b[64];
      std::snprintf(b, sizeof b, ", \"probe_max_speed\": %.9g", probeMaxSpeed);
      probeJson += b;
    }
    if (mips)
      probeJson += ", \"mips\": " + std::to_string(mipLevels);
    if (!bodyLoadsHost.empty())
    {
      char b[96];
      std::snprintf(b, sizeof b, ", \"bodies\": %d, \"body_max_residual\": %.9g", bodies, bodyMaxResidual);
      probeJson += b;
      if (!bodyPosesFinal.empty())
      {
        probeJson += ", \"body_poses\": [";
        for (int k = 0; k < bodies; k++)
        {
          probeJson += k ? ", [" : "[";
          for (int j = 0; j < 20; j++)
          {
            std::snprintf(b, sizeof b, "%s%.9g", j ? ", " : "", bodyPosesFinal[20 * (size_t)k + j]);
            probeJson += b;
          }
          probeJson += "]";
        }
        probeJson += "]";
      }
    }
    if (!rayHitsHost.empty())
      probeJson += ", \"rays\": " + std::to_string(rays) + ", \"ray_hits\": " + std::to_string(rayHitCount);
    if (!imageHost.empty())
      probeJson += ", \"image_hits\": " + std::to_string(imageHits);
    std::printf("{\"app\": \"waveapp_headless\", \"n\": %d, \"cascades\": 3, \"frames\": %d, \"frozen_frames\": %d, "
                "\"reseeded_frames\": %d, \"reseed\": \"%s\", \"mesh_vertices\": %lld, \"seconds\": %.6f, "
                "\"ms_per_frame\": %.6f, \"frames_per_s\": %.3f, \"height_field_points_per_s\": %.6e, "
                "\"final_time\": [%.9g, %.9g, %.9g]%s}\n",
                n, frames, frozen, reseeds, reseed_every_frame ? "reference (every frame)" : "on-edit",
                mesh > 0 ? (long long)(mesh + 1) * (mesh + 1) : 0LL, secs, 1e3 * secs / frames, frames / secs,
                3.0 * n * n * frames / secs, generators[0]->GetOceanSettings().time,
                generators[1]->GetOceanSettings().time, generators[2]->GetOceanSettings().time, probeJson.c_str());
    delete hulls;
    if (posesDevice)
      (void)hipFree(posesDevice);
    if (raysDevice)
      (void)hipFree(raysDevice);
    for (auto* g : generators)
      delete g;
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "waveapp_headless: %s\n", e.what());
    return 1;
  }
  return 0;
}
