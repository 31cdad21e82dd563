// Generator.cpp — Waves::Generator over the C ABI (reference src/Generator.cpp).
#include "waves/Generator.h"

#include <stdexcept>
#include <string>

namespace Waves
{

static_assert(sizeof(GeneratorSettings) == sizeof(ocean_settings), "settings layout");

Generator::Generator(Vision::RenderDevice* device, FFTCalculator* calc)
  : renderDevice(device), fftCalc(calc), textureSize(calc ? calc->GetTextureResolution() : 0)
{
  if (!device || !calc)
    throw std::runtime_error("Waves::Generator: null RenderDevice or FFTCalculator");
  if (ocean_generator_create(&gen, calc->GetPlan(), 1) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator: ") + ocean_last_error());
  // The generator's HBM maps, exposed as Vision IDs (src/Generator.cpp:99-133).
  const std::size_t n = textureSize;
  heightMap = renderDevice->RegisterTexture2D(ocean_generator_height_map(gen, 0), n, n,
                                              Vision::PixelType::RGBA32Float);
  displacementMap = renderDevice->RegisterTexture2D(ocean_generator_displacement_map(gen, 0), n, n,
                                                    Vision::PixelType::RGBA32Float);
  jacobian = renderDevice->RegisterTexture2D(ocean_generator_jacobian_map(gen, 0), n, n,
                                             Vision::PixelType::R32Float);
}

Generator::~Generator()
{
  renderDevice->DestroyTexture2D(heightMap);
  renderDevice->DestroyTexture2D(displacementMap);
  renderDevice->DestroyTexture2D(jacobian);
  for (const auto* mips : {&heightMips, &displacementMips, &jacobianMips})
    for (Vision::ID id : *mips)
      renderDevice->DestroyTexture2D(id);
  DropKinematicsMaps();
  for (Vision::ID id : {heightRateMap, displacementRateMap, foamMap})
    if (id)
      renderDevice->DestroyTexture2D(id);
  ocean_generator_destroy(gen);
}

GeneratorSettings& Generator::GetOceanSettings()
{
  return *reinterpret_cast<GeneratorSettings*>(ocean_generator_settings(gen, 0));
}

void Generator::CalculateOcean(float timestep, bool updateOcean)
{
  if (ocean_generator_calculate(gen, timestep, updateOcean ? 1 : 0) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator::CalculateOcean: ") + ocean_last_error());
}

void Generator::GenerateMips()
{
  if (ocean_generator_build_mips(gen) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator::GenerateMips: ") + ocean_last_error());
  if (!heightMips.empty())
    return;
  for (int level = 1; level < GetMipLevels(); level++)
  {
    const std::size_t side = textureSize >> level;
    heightMips.push_back(renderDevice->RegisterTexture2D(ocean_generator_height_mip(gen, 0, level), side, side,
                                                         Vision::PixelType::RGBA32Float));
    displacementMips.push_back(renderDevice->RegisterTexture2D(ocean_generator_displacement_mip(gen, 0, level), side,
                                                               side, Vision::PixelType::RGBA32Float));
    jacobianMips.push_back(renderDevice->RegisterTexture2D(ocean_generator_jacobian_mip(gen, 0, level), side, side,
                                                           Vision::PixelType::R32Float));
  }
}

Vision::ID Generator::Mip(const std::vector<Vision::ID>& mips, Vision::ID map, int level) const
{
  if (level == 0)
    return map;
  if (level < 0 || level >= GetMipLevels())
    throw std::runtime_error("Waves::Generator: mip level outside 0..log2(N)");
  if (mips.empty())
    throw std::runtime_error("Waves::Generator: the mip pyramid was never built (GenerateMips)");
  return mips[(std::size_t)level - 1];
}

void Generator::CalculateRates()
{
  if (ocean_generator_calculate_rates(gen) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator::CalculateRates: ") + ocean_last_error());
  if (heightRateMap)
    return;
  const std::size_t n = textureSize;
  heightRateMap = renderDevice->RegisterTexture2D(ocean_generator_height_rate_map(gen, 0), n, n,
                                                  Vision::PixelType::RGBA32Float);
  displacementRateMap = renderDevice->RegisterTexture2D(ocean_generator_displacement_rate_map(gen, 0), n, n,
                                                        Vision::PixelType::RGBA32Float);
}

Vision::ID Generator::Rate(Vision::ID map) const
{
  if (!map)
    throw std::runtime_error("Waves::Generator: the rates were never calculated (CalculateRates)");
  return map;
}

void Generator::DropKinematicsMaps()
{
  for (Vision::ID id : kinematicsMaps)
    renderDevice->DestroyTexture2D(id);
  kinematicsMaps.clear();
}

void Generator::SetDepthLayers(const float* depths, int layers)
{
  const int before = ocean_generator_depth_layers(gen, nullptr);
  if (ocean_generator_set_depth_layers(gen, depths, layers) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator::SetDepthLayers: ") + ocean_last_error());
  if (layers != before)  // the library freed the storage the IDs name
    DropKinematicsMaps();
}

void Generator::CalculateKinematics()
{
  if (ocean_generator_calculate_kinematics(gen) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator::CalculateKinematics: ") + ocean_last_error());
  if (!kinematicsMaps.empty())
    return;
  const std::size_t n = textureSize;
  const int layers = ocean_generator_depth_layers(gen, nullptr);
  for (int layer = 0; layer < layers; layer++)
    for (int image = 0; image < 2; image++)
      kinematicsMaps.push_back(renderDevice->RegisterTexture2D(ocean_generator_kinematics_map(gen, 0, layer, image), n, n,
                                                               Vision::PixelType::RGBA32Float));
}

Vision::ID Generator::GetKinematicsMap(int layer, int image) const
{
  if (kinematicsMaps.empty())
    throw std::runtime_error("Waves::Generator: the depth layers were never calculated (CalculateKinematics)");
  if (layer < 0 || (std::size_t)layer >= kinematicsMaps.size() / 2 || image < 0 || image > 1)
    throw std::runtime_error("Waves::Generator: depth layer or image out of range");
  return kinematicsMaps[(std::size_t)layer * 2 + image];
}

void Generator::BuildBounds()
{
  if (ocean_generator_build_bounds(gen) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator::BuildBounds: ") + ocean_last_error());
}

void Generator::GetBounds(float out[18]) const
{
  if (ocean_generator_bounds(gen, 0, out) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator::GetBounds: ") + ocean_last_error());
}

void Generator::AdvanceFoam(float dt)
{
  if (ocean_generator_advance_foam(gen, dt) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator::AdvanceFoam: ") + ocean_last_error());
}

void Generator::ResetFoam()
{
  if (ocean_generator_reset_foam(gen) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator::ResetFoam: ") + ocean_last_error());
}

ocean_foam_settings& Generator::GetFoamSettings() { return *ocean_generator_foam_settings(gen, 0); }

Vision::ID Generator::GetFoamMap()
{
  if (foamMap)
    return foamMap;
  float* map = ocean_generator_foam_map(gen, 0);
  if (!map)
    throw std::runtime_error(std::string("Waves::Generator::GetFoamMap: ") + ocean_last_error());
  foamMap = renderDevice->RegisterTexture2D(map, textureSize, textureSize, Vision::PixelType::R32Float);
  return foamMap;
}

void Generator::GetFoamCounts(int64_t out[3]) const
{
  if (ocean_generator_foam_counts(gen, 0, out) != OCEAN_OK)
    throw std::runtime_error(std::string("Waves::Generator::GetFoamCounts: ") + ocean_last_error());
}

void Generator::LoadShaders(bool) {}

}  // namespace Waves
