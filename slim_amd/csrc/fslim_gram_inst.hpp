// fslim_gram_inst.hpp -- what engine.hip needs of the item-space FSLIM kernels (cd_fslim_gram.hpp,
// instantiated in fslim_gram_inst.hip): their arguments beyond SolveArgs, and the kernels themselves.
#pragma once
#include "tile_inst.hpp"

namespace slimamd {

// One slice of the work list: positions [pos0, pos0 + npos), pos0 a multiple of 32 (whole tiles).
// Everything below is indexed by the position INSIDE the slice; so are S.ulist / S.tile_nunion.
struct FslimArgs {
  int32_t pos0, npos;
  int32_t stride;     // entries per neighbour list: min(nnbrs, ncols - 1) rounded up to 64
  int32_t* nbr_n;     // [npos]          nn = min(#candidates, nnbrs)
  int32_t* nbr_id;    // [npos][stride]  neighbour ids, ascending
  float* nbr_aty;     // [npos][stride]  G[item][neighbour]
  int32_t* nbr_slot;  // [npos][stride]  the neighbour's slot in the tile's union list
  int32_t wave_lds;   // solver: bytes of dynamic LDS per wavefront (a multiple of 16)
  int32_t tab_n;      // solver, block form: entries of the slot -> j table (>= any nunion)
};

using FslimFn = void (*)(const DevMatrix, const SolveArgs, const FslimArgs);

constexpr int kFslimMaxNbrs = 4096;     // neighbours per problem the solver's LDS state holds
constexpr int kFslimSelectThreads = 256;
constexpr int kFslimUnionThreads = 256;
constexpr int kFslimBlockMaxStride = 128;  // largest stride whose nn x nn block of G is kept in LDS
constexpr int kFslimMaxWaves = 8;          // wavefronts per solver workgroup, at most

FslimFn fslim_select_fn();
FslimFn fslim_union_fn();
FslimFn fslim_solve_fn(bool block_in_lds);
// dynamic LDS of the union kernel (item bitmap + per-word ranks) and of one solver wavefront
size_t fslim_union_lds(int ncols);
size_t fslim_wave_lds(int stride, bool block_in_lds, int tab_n);

}  // namespace slimamd
