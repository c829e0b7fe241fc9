// cd_fslim_gram.hpp -- FSLIM (nnbrs > 0; estimate.c:424-431, neighbors.c:16-125) in item space.
//
// The tile kernel's FSLIM form (cd_tile.hpp) runs a whole screen pass over R to get 32 rows of
// G = R^T R, selects in them, and then sweeps over <= nnbrs coordinates per problem: nearly all of
// its time goes into the rows.  With the float G on the handle (cd_gram.hpp) the rows are there:
//
//   select : row iC of G holds a_i . a_iC for every i.  With ratings all > 0 the co-rated columns
//            (neighbors.c:46-60) are exactly {i != iC : G[iC][i] > 0}; their similarity is the tile
//            kernel's float expression, the nnbrs largest are found by the same 4-pass radix select
//            over the same sortable keys, ties at the cut going to the lower ids
//            (slim_oracle.c:340-351).  One workgroup per problem, the row re-read from L2 per pass.
//   union  : the ascending union of a tile's <= 32 lists (the order contract below), and for every
//            neighbour its slot in it.  One workgroup per tile, an LDS bitmap over the items.
//   solve  : the problem lives on nn <= nnbrs coordinates: g_j = aTy_j - sum_k B[j][k] x_k with
//            B = G[nbrs, nbrs].  One WAVEFRONT per problem (the descent is serial in the coordinate),
//            several per workgroup, each pulling positions off the queue; x, g and the neighbours'
//            scalars in LDS.  B is gathered once into LDS when nn^2 floats fit the wavefront's share
//            (block form), else G[nbr_f][nbr_k] is gathered per update (gathered form): the same
//            values, the same fmaf sequence, the same bits.
//
// Order contract: sweep t of a problem walks perm(nunion, key(seed, gkey, t)) over its TILE's union
// and skips the slots outside its own list -- cd_tile.hpp's FSLIM order, so the oracle's tile walk
// checks it visit for visit.  The update arithmetic is cd_gram.hpp's (cd_wave.hpp helpers).
// A warm start is ignored: the reference's FSLIM branch never sets its warm-start flags.
#pragma once
#include "cd_tile.hpp"
#include "fslim_gram_inst.hpp"

namespace slimamd {

// order-preserving map float -> uint32 (cd_tile.hpp's keyof); +inf sorts above every finite value
__device__ __forceinline__ uint32_t fslim_key(const float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// candidate test and similarity key of column i for problem `item` (cd_tile.hpp:720-725)
__device__ __forceinline__ bool fslim_cand_key(const DevMatrix& A, const int simtype, const int item,
                                               const float cn_item, const int i, const float a, uint32_t& key) {
  if (i >= A.ncols || i == item || !(a > 0.0f)) return false;
  const float cn_i = A.cnorm[i];
  const float sim = simtype == 0 ? a / cn_i : (simtype == 1 ? a / ((cn_i + cn_item) - a) : a);
  key = fslim_key(sim);
  return true;
}

__global__ __launch_bounds__(kFslimSelectThreads) void fslim_gram_select_kernel(const DevMatrix A, const SolveArgs S,
                                                                               const FslimArgs F) {
  constexpr int NT = kFslimSelectThreads, NW = NT / 64;
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_prefix, s_want;
  __shared__ int s_above[NW], s_ties[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
  const uint64_t lane_lt = (1ull << lane) - 1ull;
  const int lp = blockIdx.x;
  if (lp >= F.npos) return;
  const int item = uni(S.order[F.pos0 + lp]);
  const float* __restrict__ row = S.G + (int64_t)item * S.G_ld;
  const float4* __restrict__ row4 = reinterpret_cast<const float4*>(row);
  const float cn_item = A.cnorm[item];
  const int simtype = S.simtype;
  const int n4 = S.ncols_pad >> 2;
  if (tid == 0) {
    s_prefix = 0u;
    s_want = (uint32_t)S.nnbrs;
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t hi_mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    hist[tid] = 0u;
    __syncthreads();
    const uint32_t prefix = s_prefix;
    for (int c = tid; c < n4; c += NT) {
      const float4 a4 = row4[c];
      if (!(a4.x > 0.0f || a4.y > 0.0f || a4.z > 0.0f || a4.w > 0.0f)) continue;
      const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uint32_t key = 0u;
        if (fslim_cand_key(A, simtype, item, cn_item, 4 * c + e, av[e], key) && (key & hi_mask) == prefix)
          atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (tid == 0) {  // walk the digits from the top until `want` entries are covered
      uint32_t want = s_want, d = 255u;
      for (;; --d) {
        const uint32_t c = hist[d];
        if (c >= want || d == 0u) break;
        want -= c;
      }
      // fewer candidates than wanted: the walk ends at digit 0 and everything is taken
      s_prefix = prefix | (d << shift);
      s_want = want;
    }
    __syncthreads();
  }
  // T = the threshold key, quota = entries equal to T to keep, lowest ids first.  Every wavefront
  // owns a contiguous piece of the row: count, exchange, then compact in id order with ballots.
  const uint32_t T = s_prefix;
  const int quota = (int)s_want;
  const int seg = ((S.ncols_pad / 64 + NW - 1) / NW) * 64;
  const int i0 = wave * seg, i1 = (i0 + seg) < S.ncols_pad ? (i0 + seg) : S.ncols_pad;
  int above = 0, ties = 0;
  for (int ib = i0; ib < i1; ib += 64) {
    const int i = ib + lane;
    uint32_t key = 0u;
    const bool cand = fslim_cand_key(A, simtype, item, cn_item, i, row[i], key);
    above += __popcll(__ballot(cand && key > T));
    ties += __popcll(__ballot(cand && key == T));
  }
  if (lane == 0) {
    s_above[wave] = above;
    s_ties[wave] = ties;
  }
  __syncthreads();
  int out = 0, ties_before = 0, total_above = 0, total_ties = 0;
  for (int w = 0; w < NW; ++w) {
    if (w < wave) {
      out += s_above[w];
      ties_before += s_ties[w];
    }
    total_above += s_above[w];
    total_ties += s_ties[w];
  }
  const int taken_before = ties_before < quota ? ties_before : quota;
  out += taken_before;
  int left = quota - taken_before;
  int32_t* __restrict__ oid = F.nbr_id + (int64_t)lp * F.stride;
  float* __restrict__ oaty = F.nbr_aty + (int64_t)lp * F.stride;
  for (int ib = i0; ib < i1; ib += 64) {
    const int i = ib + lane;
    const float a = row[i];
    uint32_t key = 0u;
    const bool cand = fslim_cand_key(A, simtype, item, cn_item, i, a, key);
    const bool tie = cand && key == T;
    const uint64_t mt = __ballot(tie);
    const bool act = cand && (key > T || (tie && __popcll(mt & lane_lt) < left));
    left -= __popcll(mt) < left ? __popcll(mt) : left;
    const uint64_t ma = __ballot(act);
    const int dst = out + __popcll(ma & lane_lt);
    if (act && dst < F.stride) {
      oid[dst] = i;
      oaty[dst] = a;
    }
    out += __popcll(ma);
  }
  if (tid == 0) {
    const int nn = total_above + (total_ties < quota ? total_ties : quota);
    F.nbr_n[lp] = nn < F.stride ? nn : F.stride;
  }
}

// The ascending union of a tile's lists and every neighbour's slot in it.
__global__ __launch_bounds__(kFslimUnionThreads) void fslim_gram_union_kernel(const DevMatrix A, const SolveArgs S,
                                                                             const FslimArgs F) {
  constexpr int NT = kFslimUnionThreads;
  extern __shared__ uint32_t fu_lds[];  // [nw] item bitmap, [nw] members before each word
  __shared__ int s_cnt[NT];
  __shared__ int s_total;
  const int tid = threadIdx.x;
  const int nw = (A.ncols + 31) >> 5;
  uint32_t* const bm = fu_lds;
  uint32_t* const rank = fu_lds + nw;
  const int grp = blockIdx.x;
  const int base = grp * 32;
  const int nprob = (F.npos - base) < 32 ? (F.npos - base) : 32;
  int* __restrict__ ul = S.ulist + (int64_t)grp * S.u_stride;
  for (int w = tid; w < nw; w += NT) bm[w] = 0u;
  __syncthreads();
  for (int q = 0; q < nprob; ++q) {
    const int nn = F.nbr_n[base + q];
    const int32_t* __restrict__ ids = F.nbr_id + (int64_t)(base + q) * F.stride;
    for (int j = tid; j < nn; j += NT) {
      const int id = ids[j];
      atomicOr(&bm[id >> 5], 1u << (id & 31));
    }
  }
  __syncthreads();
  const int chunk = (nw + NT - 1) / NT;
  const int w0 = tid * chunk < nw ? tid * chunk : nw, w1 = (w0 + chunk) < nw ? (w0 + chunk) : nw;
  int c = 0;
  for (int w = w0; w < w1; ++w) c += __popc(bm[w]);
  s_cnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < NT; ++t) {
      const int v = s_cnt[t];
      s_cnt[t] = run;
      run += v;
    }
    s_total = run;
  }
  __syncthreads();
  int r = s_cnt[tid];
  for (int w = w0; w < w1; ++w) {
    rank[w] = (uint32_t)r;
    uint32_t bits = bm[w];
    while (bits) {
      const int b = __builtin_ctz(bits);
      bits &= bits - 1u;
      if (r < S.u_stride) ul[r] = w * 32 + b;
      ++r;
    }
  }
  __syncthreads();
  for (int q = 0; q < nprob; ++q) {
    const int nn = F.nbr_n[base + q];
    const int32_t* __restrict__ ids = F.nbr_id + (int64_t)(base + q) * F.stride;
    int32_t* __restrict__ slots = F.nbr_slot + (int64_t)(base + q) * F.stride;
    for (int j = tid; j < nn; j += NT) {
      const int id = ids[j];
      slots[j] = (int)rank[id >> 5] + __popc(bm[id >> 5] & ((1u << (id & 31)) - 1u));
    }
  }
  if (tid == 0) S.tile_nunion[grp] = s_total;
}

// BLOCK: B = G[nbrs, nbrs] in LDS (row stride F.stride) and a slot -> j table; else B's entries are
// gathered from G per update and the slot is looked up by binary search.
template <bool BLOCK>
__global__ __launch_bounds__(64 * kFslimMaxWaves) void cd_fslim_gram_kernel(const DevMatrix A, const SolveArgs S,
                                                                           const FslimArgs F) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fs_lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = uni(tid >> 6);
  const uint64_t lane_lt = (1ull << lane) - 1ull;
  const int st = F.stride;
  // this wavefront's share: x, g, |a_i|^2, cnorm, nnz, union slot, id of the neighbours; the queue
  // of compacted visits; (block form) the slot -> j table and B
  float* const x = reinterpret_cast<float*>(fs_lds + (size_t)wave * (size_t)F.wave_lds);
  float* const g = x + st;
  float* const sq = g + st;
  float* const cn = sq + st;
  int* const len = reinterpret_cast<int*>(cn + st);
  int* const slot = len + st;
  int* const id = slot + st;
  int* const qj = id + st;  // [128]
  uint16_t* const tab = reinterpret_cast<uint16_t*>(qj + 128);
  float* const B = reinterpret_cast<float*>(tab + (BLOCK ? F.tab_n : 0));
  const float l1 = S.l1, l2 = S.l2;
  const float* __restrict__ Gm = S.G;
  const int64_t ld = S.G_ld;
  const int64_t* __restrict__ colptr = A.colptr;

  for (;;) {
    // Every lane takes part in the pull (63 of them add 0).  Written as `if (lane == 0) lp =
    // atomicAdd(..)`, the compiler joined that branch to the `if (lane == 0)` that ends the
    // iteration before it: lane 0 stored, pulled and waited in an outer loop while the other 63
    // lanes went round an inner loop that never pulls -- on the same position, for ever (seen in
    // the assembly).  Without a branch at the head there is nothing to join.
    const int lp = lane_bcast(atomicAdd(S.queue, lane == 0 ? 1 : 0), 0);
    if (lp >= F.npos) break;
    const int p = F.pos0 + lp;
    const int item = uni(S.order[p]);
    // position of the item's tile in the unsharded work list (cd_gram.hpp: gkey)
    const uint32_t gkey = (uint32_t)((p >> 5) * S.shard_count + S.shard_index);
    const int nunion = uni(S.tile_nunion[lp >> 5]);
    const int nn = uni(F.nbr_n[lp]);
    const int32_t* __restrict__ nid = F.nbr_id + (int64_t)lp * st;
    const float* __restrict__ naty = F.nbr_aty + (int64_t)lp * st;
    const int32_t* __restrict__ nslot = F.nbr_slot + (int64_t)lp * st;

    wave_sync<true>();  // (the previous problem's reads of the share are done)
    if (BLOCK)
      for (int t = lane; t < nunion; t += 64) tab[t] = (uint16_t)0xFFFFu;
    wave_sync<true>();
    for (int j = lane; j < nn; j += 64) {
      const int i = nid[j];
      id[j] = i;
      x[j] = 0.0f;
      g[j] = naty[j];
      sq[j] = A.csq[i];
      cn[j] = A.cnorm[i];
      len[j] = (int)(colptr[i + 1] - colptr[i]);
      const int s = nslot[j];
      slot[j] = s;
      if (BLOCK) tab[s] = (uint16_t)j;
    }
    wave_sync<true>();
    if (BLOCK) {
      for (int j = 0; j < nn; ++j) {
        const float* __restrict__ grow = Gm + (int64_t)id[j] * ld;
        for (int k = lane; k < nn; k += 64) B[j * st + k] = grow[id[k]];
      }
      wave_sync<true>();
    }

    int maxit = 0;
    {
      const int64_t cap = 50 * (uni(colptr[item + 1]) - uni(colptr[item]));  // estimate.c:448-449
      maxit = cap < (int64_t)S.maxniters ? (int)cap : S.maxniters;
    }
    int niters = 0, conv = 0;
    unsigned long long Dq = 0, Uq = 0;  // per lane
    float dlt = 0.0f;

    // up to 64 visits, lane L holding visit L of the batch (coordinate jq, or none): every lane decides
    // against the g it holds; the first lane whose coefficient moves is the next change of the
    // sequential algorithm; it is applied to g, every lane reads its g again (cd_gram.hpp:413-460)
    auto run_batch = [&](const int jq, const bool part) {
      float xi = 0.0f, gi = 0.0f, sqi = 0.0f, cni = 1.0f;
      int leni = 0, idi = 0;
      if (part) {
        xi = x[jq];
        gi = g[jq];
        sqi = sq[jq];
        cni = cn[jq];
        leni = len[jq];
        idi = id[jq];
      }
      Dq += (unsigned long long)leni;
      uint64_t pend = __ballot(part);
      while (pend) {
        const float xeff = (xi > kEps || xi < -kEps) ? xi : 0.0f;
        const float num = cd_num(gi, xeff, sqi);
        const float nx = num > l1 ? (num - l1) / cd_den(cni, l2) : 0.0f;
        const float neff = (nx > kEps || nx < -kEps) ? nx : 0.0f;
        const float d = neff - xeff;
        const uint64_t m = __ballot(part && nx != xi) & pend;
        const int f = m ? __builtin_ctzll(m) : 64;
        // visits decided by now: the ones ahead of f kept their coefficient, f moves.  A visit
        // touches the column when the old or the new coefficient is not 0 (slim_oracle.c:900-909)
        const bool settled = part && ((pend >> lane) & 1ull) && lane <= f;
        if (settled && (xeff != 0.0f || neff != 0.0f)) Uq += (unsigned long long)leni;
        if (m == 0) break;
        const int j_f = lane_bcast(jq, f);
        const int id_f = lane_bcast(idi, f);
        const float d_f = lane_bcast(d, f);
        dlt = fmaf(d_f, d_f, dlt);
        if (lane == f) x[jq] = nx;
        pend = f == 63 ? 0ull : (pend & ~((2ull << f) - 1ull));
        if (d_f != 0.0f) {
          if (BLOCK) {
            const float* __restrict__ brow = B + j_f * st;
            for (int k = lane; k < nn; k += 64) g[k] = fmaf(-d_f, brow[k], g[k]);
          } else {
            const float* __restrict__ grow = Gm + (int64_t)id_f * ld;
            for (int k = lane; k < nn; k += 64) g[k] = fmaf(-d_f, grow[id[k]], g[k]);
          }
          wave_sync<true>();
          if (part) gi = g[jq];
        }
      }
      wave_sync<true>();
    };

    for (int t = 0;; ++t) {
      if (t >= maxit) {  // loop exhausted without convergence: niters = t + 1 (cd.c:140)
        niters = maxit + 1;
        break;
      }
      dlt = 0.0f;
      const PermCtx pc = perm_make((uint32_t)nunion, perm_key(S.seed, gkey, (uint32_t)t));
      int cnt = 0;  // own coordinates found and not yet visited, in position order (qj)
      for (int p0 = 0; p0 < nunion; p0 += 64) {
        const int pos = p0 + lane;
        int j = -1;
        if (pos < nunion) {
          const int u = (int)perm_index(pc, (uint32_t)pos);
          if (BLOCK) {
            const int tj = (int)tab[u];
            j = tj == 0xFFFF ? -1 : tj;
          } else {
            int lo = 0, hi = nn;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (slot[mid] < u) lo = mid + 1; else hi = mid;
            }
            j = (lo < nn && slot[lo] == u) ? lo : -1;
          }
        }
        const uint64_t mo = __ballot(j >= 0);
        if (j >= 0) qj[cnt + __popcll(mo & lane_lt)] = j;
        cnt += __popcll(mo);
        wave_sync<true>();
        const bool last = p0 + 64 >= nunion;
        while (cnt >= 64 || (last && cnt > 0)) {
          const int nb = cnt < 64 ? cnt : 64;
          const bool part = lane < nb;
          const int jq = part ? qj[lane] : 0;
          const int rest = (lane < cnt - nb) ? qj[nb + lane] : 0;
          wave_sync<true>();
          if (lane < cnt - nb) qj[lane] = rest;
          cnt -= nb;
          run_batch(jq, part);
        }
      }
      if (dlt < S.opt_tol) {  // cd.c:135-138
        conv = 1;
        niters = t + 1;
        break;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      Dq += __shfl_xor(Dq, o);
      Uq += __shfl_xor(Uq, o);
    }

    // -- 1/2 ||r||^2 and the objective in item space (cd_gram.hpp:509-538):
    //    ||y - A x||^2 = |a_iC|^2 - sum_j x_j (aTy_j + g_j)
    double e2 = 0.0, reg = 0.0;
    for (int j = lane; j < nn; j += 64) {
      const float xv = x[j];
      reg += 0.5 * (double)l2 * (double)xv * (double)xv + (double)l1 * (double)fabsf(xv);
      if (xv > kEps || xv < -kEps) e2 += (double)xv * ((double)naty[j] + (double)g[j]);
    }
    for (int o = 32; o > 0; o >>= 1) {
      e2 += __shfl_xor(e2, o);
      reg += __shfl_xor(reg, o);
    }
    const float err = (float)(0.5 * ((double)A.csq[item] - e2));

    // -- output: |x| > 1e-7, ids ascending already (estimate.c:492-505; cd_gram.hpp:531-576)
    int nz = 0;
    for (int jb = 0; jb < nn; jb += 64) {
      const int j = jb + lane;
      nz += __popcll(__ballot(j < nn && fabsf(x[j]) > kEps));
    }
    unsigned long long off = 0;
    if (lane == 0) off = atomicAdd(S.out_cursor, (unsigned long long)nz);
    off = (unsigned long long)uni((int64_t)off);
    const bool fits = (int64_t)(off + (unsigned long long)nz) <= S.out_cap;
    if (fits) {
      int wpos = 0;
      for (int jb = 0; jb < nn; jb += 64) {
        const int j = jb + lane;
        const float xv = j < nn ? x[j] : 0.0f;
        const bool keep = j < nn && fabsf(xv) > kEps;
        const uint64_t m = __ballot(keep);
        if (keep) {
          const int64_t dst = (int64_t)off + wpos + __popcll(m & lane_lt);
          S.out_ind[dst] = id[j];
          S.out_val[dst] = xv;
        }
        wpos += __popcll(m);
      }
    }
    if (lane == 0) {
      if (!fits) atomicMax(S.overflow, 1);
      S.out_cnt[item] = fits ? nz : -nz - 1;
      S.out_off[item] = (int64_t)off;
      S.st_na[item] = nn;
      S.st_sweeps[item] = niters;
      S.st_conv[item] = conv;
      S.st_D[item] = (int64_t)Dq;
      S.st_U[item] = (int64_t)Uq;
      S.st_G[item] = 0;  // (the engine reports the staging pass's G for the column)
      S.st_err[item] = err;
      S.st_obj[item] = err + (float)reg;
    }
  }
}

}  // namespace slimamd
