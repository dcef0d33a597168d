// fdoct_grid.h -- launch arithmetic the *_kernels.h launchers share: the cap of a grid-stride kernel's grid (256 CUs if unknown).
#pragma once
namespace fdoct {
constexpr int resident_blocks(int num_cu, int waves_per_cu, int block) { return (num_cu > 0 ? num_cu : 256) * (waves_per_cu / (block / 64)); }
}  // namespace fdoct
