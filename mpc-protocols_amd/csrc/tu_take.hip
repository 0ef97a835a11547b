#include "kernels_take.hpp"
#include "launchers.hpp"
namespace hbmpc {
// one launch for the first `count` slices of `a`: tiles = the longest slice's tiles, the rows in the grid's y, the slice in its z
void launch_take_rows(int ew64, const TakeArgs& a, unsigned tiles, unsigned rows, unsigned count, hipStream_t s) {
    const dim3 grid(tiles, rows, count);
    if (ew64 == 4) hipLaunchKernelGGL(k_take_rows<4>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_take_rows<1>, grid, dim3(256), 0, s, a);
}
}
