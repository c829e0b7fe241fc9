// fslim_gram_select_kernel, fslim_gram_union_kernel and cd_fslim_gram_kernel<BLOCK>; see
// fslim_gram_inst.hpp
#include "cd_fslim_gram.hpp"
namespace slimamd {
FslimFn fslim_select_fn() { return fslim_gram_select_kernel; }
FslimFn fslim_union_fn() { return fslim_gram_union_kernel; }
FslimFn fslim_solve_fn(bool block_in_lds) {
  return block_in_lds ? cd_fslim_gram_kernel<true> : cd_fslim_gram_kernel<false>;
}
size_t fslim_union_lds(int ncols) { return 2 * sizeof(uint32_t) * (size_t)((ncols + 31) / 32); }
// x, g, |a_i|^2, cnorm, nnz, slot, id of `stride` neighbours + the 128-entry visit queue; the block
// form adds the 16-bit slot -> j table and the stride x stride block of G
size_t fslim_wave_lds(int stride, bool block_in_lds, int tab_n) {
  size_t b = 7 * sizeof(float) * (size_t)stride + 128 * sizeof(int32_t);
  if (block_in_lds) b += sizeof(uint16_t) * (size_t)tab_n + sizeof(float) * (size_t)stride * (size_t)stride;
  return (b + 15) / 16 * 16;
}
}  // namespace slimamd
