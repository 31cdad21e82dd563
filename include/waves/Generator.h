// waves/Generator.h — drop-in for Waves::Generator / Waves::GeneratorSettings
// (reference src/Generator.h:12-93). Same members and semantics; the GLSL kernels are replaced by
// the fused HIP row/column passes of liboceanfft.
#pragma once

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "oceanfft.h"
#include "vision/RenderDevice.h"
#include "waves/FFTCalculator.h"

namespace Waves
{

// glm::ivec2 stand-in with the same layout (the reference's only glm use in the settings,
// src/Generator.h:14). It converts to and from any {x, y} vector type, so reference code that
// writes `settings.seed = glm::ivec2(a, b)` (or reads it back into one) compiles unchanged.
struct IVec2
{
  int32_t x = 0, y = 0;

  constexpr IVec2() = default;
  constexpr IVec2(int32_t x_, int32_t y_) : x(x_), y(y_) {}
  template <class V, class = decltype(std::declval<const V&>().x + std::declval<const V&>().y),
            class = std::enable_if_t<!std::is_same<std::decay_t<V>, IVec2>::value>>
  constexpr IVec2(const V& v) : x(static_cast<int32_t>(v.x)), y(static_cast<int32_t>(v.y))
  {
  }
  template <class V, class = decltype(V{int32_t{}, int32_t{}})>
  constexpr explicit operator V() const
  {
    return V{x, y};
  }
  int32_t& operator[](int i) { return i == 0 ? x : y; }
  const int32_t& operator[](int i) const { return i == 0 ? x : y; }
  friend constexpr bool operator==(const IVec2& a, const IVec2& b) { return a.x == b.x && a.y == b.y; }
  friend constexpr bool operator!=(const IVec2& a, const IVec2& b) { return !(a == b); }
};
static_assert(sizeof(IVec2) == 8 && std::is_trivially_copyable<IVec2>::value, "IVec2 must match glm::ivec2");

// src/Generator.h:12-30 — identical defaults and 64-byte layout.
struct GeneratorSettings
{
  IVec2 seed = {12342, 8934};  // The seed for random generation.

  float U_10 = 40.0f;         // The speed of the wind.
  float theta_0 = 25.0f;      // The CCW direction of the wind rel. to +x-axis.
  float F = 800000.0f;        // The distance to a downwind shore (fetch).
  float g = 9.8f;             // The acceleration due to gravity.
  float swell = 0.5f;         // The factor of non-wind based waves.
  float h = 100.0f;           // The depth of the ocean.
  float displacement = 0.4f;  // The scalar used in displacing the vertices.
  float time = 0.0f;          // The time in seconds since the program began.
  float planeSize = 40.0f;    // The size of the plane in meters that this plane is simulating.
  float scale = 1.0f;         // The global heightmap scalar.
  float spread = 0.2f;        // The intensity of waves perp. to wind.
  int boundWavelength = 0;    // Whether or not we bound the wavelength (1 = bound, 0 = unbound)
  float wavelengthMin = 0.0f; // The minimum wavelength that is allowed
  float wavelengthMax = 0.0f; // The maximum wavelength that is allowed
};
static_assert(sizeof(GeneratorSettings) == 64, "GeneratorSettings must stay 64 bytes (std140 UBO)");

class Generator
{
public:
  // src/Generator.h:36-37
  Generator(Vision::RenderDevice* device, FFTCalculator* calc);
  ~Generator();
  Generator(const Generator&) = delete;
  Generator& operator=(const Generator&) = delete;

  // src/Generator.h:41. If the spectrum is modified, pass updateOcean = true to the next call.
  GeneratorSettings& GetOceanSettings();

  // src/Generator.h:45. time += timestep; (re)seed h0 if requested or first call; evolve, 2D iFFT
  // of both packed maps, Jacobian. Enqueued on the device's stream (no host sync).
  void CalculateOcean(float timestep, bool updateOcean = false);

  // src/Generator.h:48-50. heightMap = (h, dh/dx, dh/dz, Dx), displacementMap =
  // (Dz, dDx/dx, dDz/dz, dDx/dz), jacobian = R32F. IDs resolve through the RenderDevice.
  Vision::ID GetHeightMap() const { return heightMap; }
  Vision::ID GetDisplacementMap() const { return displacementMap; }
  Vision::ID GetJacobianMap() const { return jacobian; }

  // src/Generator.h:53. Kernels are compiled into liboceanfft for gfx950; nothing to reload.
  void LoadShaders(bool reload = false);

  // Extension (no reference counterpart): the C-ABI generator behind this object, for ABI calls
  // such as ocean_surface_sample_plane (waves/Surface.h).
  ocean_generator* GetHandle() const { return gen; }

  // Extension (no reference counterpart; the reference builds no mip chain, src/Generator.cpp:116-119):
  // the box-filter pyramid of the three maps (ocean_generator_build_mips, oceanfft.h), what
  // glGenerateMipmap would give. GenerateMips enqueues the rebuild of levels 1 .. GetMipLevels() - 1
  // from the current maps on the device's stream; call it after CalculateOcean and before
  // SurfaceSampler::SampleLod. Level 0 of a getter is the map itself, level l an image of side N >> l;
  // the getters throw before the first GenerateMips and for a level out of range.
  void GenerateMips();
  int GetMipLevels() const { return ocean_generator_mip_levels(gen); }
  Vision::ID GetHeightMip(int level) const { return Mip(heightMips, heightMap, level); }
  Vision::ID GetDisplacementMip(int level) const { return Mip(displacementMips, displacementMap, level); }
  Vision::ID GetJacobianMip(int level) const { return Mip(jacobianMips, jacobian, level); }

  // Extension (no reference counterpart): the time derivative of heightMap and displacementMap at the
  // time of the last CalculateOcean (ocean_generator_calculate_rates, oceanfft.h), channel for channel:
  // d/dt (h, dh/dx, dh/dz, Dx) and d/dt (Dz, dDx/dx, dDz/dz, dDx/dz). CalculateRates enqueues it on the
  // device's stream; call it after CalculateOcean and before SurfaceSampler::Velocity. The getters throw
  // before the first CalculateRates.
  void CalculateRates();
  Vision::ID GetHeightRateMap() const { return Rate(heightRateMap); }
  Vision::ID GetDisplacementRateMap() const { return Rate(displacementRateMap); }

  // Extension (no reference counterpart): the water below the surface (ocean_generator_set_depth_layers,
  // ocean_generator_calculate_kinematics, oceanfft.h). SetDepthLayers takes 1..8 rest depths in metres below
  // the mean water level (finite, >= 0, strictly ascending). CalculateKinematics enqueues, per depth, two
  // RGBA32F N x N maps on the device's stream: image 0 = (vertical velocity, its x-slope, partner, d/dt Dx),
  // image 1 = (d/dt Dz, partner, pressure head in m, its x-slope), each wavenumber attenuated by linear wave
  // theory's profile for that depth, both profiles 1 at the surface. Call it after CalculateOcean and before
  // SurfaceSampler::Kinematics. GetKinematicsMap throws before the first CalculateKinematics and for a layer
  // or image out of range; its IDs are registered anew after a change of the layer count.
  void SetDepthLayers(const float* depths, int layers);
  int GetDepthLayers(float out[8]) const { return ocean_generator_depth_layers(gen, out); }
  void CalculateKinematics();
  Vision::ID GetKinematicsMap(int layer, int image) const;

  // Extension (no reference counterpart): the minimum and maximum of the nine map channels
  // (ocean_generator_build_bounds, oceanfft.h): culling boxes, the slab SurfaceSampler::Raycast clips its
  // rays to, and min jacobian > 0 as the sign that SurfaceSampler::Query converges everywhere. BuildBounds
  // enqueues the reduction on the device's stream; call it after CalculateOcean and before Raycast.
  // GetBounds copies the 18 floats to the host (it waits for the stream): (min, max) of heightMap x, y, z,
  // w, displacementMap x, y, z, w and the Jacobian; it throws while the bounds are not built or stale.
  void BuildBounds();
  void GetBounds(float out[18]) const;

  // Extension (the reference declares it, src/Generator.h:88-92, and never builds it): foam accumulated per
  // texel and decaying exponentially (ocean_generator_advance_foam, oceanfft.h). AdvanceFoam(dt) enqueues
  // one step from the current Jacobian map on the device's stream: call it after CalculateOcean(dt); dt = 0
  // freezes the foam. ResetFoam zeroes it. GetFoamSettings is mutable like GetOceanSettings (bias, gain,
  // decay, level; read by the next AdvanceFoam). GetFoamMap is an R32F N x N texture registered on first
  // use; it throws before the first AdvanceFoam / ResetFoam. GetFoamCounts copies the last step's
  // (breaking, covered, saturated) texel counts to the host (it waits for the stream).
  void AdvanceFoam(float dt);
  void ResetFoam();
  ocean_foam_settings& GetFoamSettings();
  Vision::ID GetFoamMap();
  void GetFoamCounts(int64_t out[3]) const;

private:
  Vision::RenderDevice* renderDevice = nullptr;
  FFTCalculator* fftCalc = nullptr;
  std::size_t textureSize = 0;
  ocean_generator* gen = nullptr;
  Vision::ID heightMap = 0;
  Vision::ID displacementMap = 0;
  Vision::ID jacobian = 0;
  // levels >= 1 (index level - 1), registered by the first GenerateMips
  std::vector<Vision::ID> heightMips, displacementMips, jacobianMips;
  Vision::ID Mip(const std::vector<Vision::ID>& mips, Vision::ID map, int level) const;
  // registered by the first CalculateRates
  Vision::ID heightRateMap = 0, displacementRateMap = 0;
  Vision::ID Rate(Vision::ID map) const;
  // [layer][image], registered by the first CalculateKinematics after a change of the layer count
  std::vector<Vision::ID> kinematicsMaps;
  void DropKinematicsMaps();
  // registered by the first GetFoamMap
  Vision::ID foamMap = 0;
};

}  // namespace Waves
