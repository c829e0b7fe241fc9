// host_csr.cpp -- see host_csr.hpp.
#include "host_csr.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <thread>

namespace slimamd {

namespace {
thread_local std::string g_err;

template <class T>
T* xmalloc(size_t n) {
  return static_cast<T*>(std::malloc(sizeof(T) * (n ? n : 1)));
}
}  // namespace

void set_error(const std::string& msg) {
  g_err = msg;
  if (!msg.empty()) std::fprintf(stderr, "[libslim/gfx950] %s\n", msg.c_str());
}
const char* last_error() { return g_err.c_str(); }

slim_csr_t* csr_new() {
  auto* m = static_cast<slim_csr_t*>(std::calloc(1, sizeof(slim_csr_t)));
  if (m) m->nrows = m->ncols = -1;
  return m;
}

void csr_free(slim_csr_t* m) {
  if (!m) return;
  void* owned[] = {m->rowptr, m->colptr,  m->rowind,  m->colind, m->rowids, m->colids,
                   m->rlabels, m->clabels, m->rmap,   m->cmap,   m->rowval, m->colval,
                   m->rnorms,  m->cnorms,  m->rsums,  m->csums,  m->rsizes, m->csizes,
                   m->rvols,   m->cvols,   m->rwgts,  m->cwgts};
  for (void* p : owned) std::free(p);
  std::free(m);
}

int32_t max_index_plus_one(int64_t nnz, const int32_t* ind) {
  int32_t hi = -1;
  for (int64_t k = 0; k < nnz; ++k) hi = std::max(hi, ind[k]);
  return hi + 1;
}

slim_csr_t* csr_from_rows(int32_t nrows, const ssize_t* ptr, const int32_t* ind,
                          const float* val) {
  slim_csr_t* m = csr_new();
  if (!m) return nullptr;
  const int64_t nnz = ptr[nrows];
  m->nrows = nrows;
  m->ncols = max_index_plus_one(nnz, ind);
  m->rowptr = xmalloc<ssize_t>(nrows + 1);
  m->rowind = xmalloc<int32_t>(nnz);
  m->rowval = val ? xmalloc<float>(nnz) : nullptr;
  if (!m->rowptr || !m->rowind || (val && !m->rowval)) {
    csr_free(m);
    return nullptr;
  }
  std::memcpy(m->rowptr, ptr, sizeof(ssize_t) * (nrows + 1));
  std::memcpy(m->rowind, ind, sizeof(int32_t) * nnz);
  if (val) std::memcpy(m->rowval, val, sizeof(float) * nnz);
  return m;
}

void csr_build_index(slim_csr_t* m, int what) {
  // source view -> destination view
  const int32_t nsrc = what == 0 ? m->nrows : m->ncols;
  const int32_t ndst = what == 0 ? m->ncols : m->nrows;
  const ssize_t* sp = what == 0 ? m->rowptr : m->colptr;
  const int32_t* si = what == 0 ? m->rowind : m->colind;
  const float* sv = what == 0 ? m->rowval : m->colval;
  const int64_t nnz = sp[nsrc];

  ssize_t* dp = xmalloc<ssize_t>(ndst + 1);
  int32_t* di = xmalloc<int32_t>(nnz);
  float* dv = sv ? xmalloc<float>(nnz) : nullptr;
  std::fill(dp, dp + ndst + 1, 0);
  // Large models (a C5 grid step returns 77M entries 45 times over): the counting-sort transpose
  // on several host threads -- sources cut into T ranges of equal nnz, one histogram per range,
  // every range scatters from its own start offsets.  Within a destination row the sources stay
  // ascending (ranges ascending, each walked in order): the same arrays as the serial form.
  const unsigned hw = std::thread::hardware_concurrency();
  const int T = nnz >= (int64_t(1) << 22) ? (int)std::min<unsigned>(16u, std::max(1u, hw)) : 1;
  if (T > 1) {
    std::vector<int32_t> cut((size_t)T + 1, nsrc);
    cut[0] = 0;
    for (int t = 1; t < T; ++t)
      cut[(size_t)t] = (int32_t)(std::lower_bound(sp, sp + nsrc + 1, (ssize_t)(nnz / T * t)) - sp);
    std::vector<std::vector<ssize_t>> hist((size_t)T, std::vector<ssize_t>((size_t)ndst, 0));
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        ssize_t* h = hist[(size_t)t].data();
        for (ssize_t k = sp[cut[(size_t)t]]; k < sp[cut[(size_t)t + 1]]; ++k) ++h[si[k]];
      });
    for (auto& x : th) x.join();
    th.clear();
    ssize_t run = 0;
    for (int32_t d = 0; d < ndst; ++d) {  // hist[t][d] becomes range t's first slot in row d
      dp[d] = run;
      for (int t = 0; t < T; ++t) {
        const ssize_t c = hist[(size_t)t][(size_t)d];
        hist[(size_t)t][(size_t)d] = run;
        run += c;
      }
    }
    dp[ndst] = run;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        ssize_t* fill = hist[(size_t)t].data();
        for (int32_t s = cut[(size_t)t]; s < cut[(size_t)t + 1]; ++s)
          for (ssize_t k = sp[s]; k < sp[s + 1]; ++k) {
            const ssize_t slot = fill[si[k]]++;
            di[slot] = s;
            if (dv) dv[slot] = sv[k];
          }
      });
    for (auto& x : th) x.join();
  } else {
    for (int64_t k = 0; k < nnz; ++k) ++dp[si[k] + 1];
    std::partial_sum(dp, dp + ndst + 1, dp);
    std::vector<ssize_t> fill(dp, dp + ndst);
    for (int32_t s = 0; s < nsrc; ++s)
      for (ssize_t k = sp[s]; k < sp[s + 1]; ++k) {
        const ssize_t slot = fill[si[k]]++;
        di[slot] = s;
        if (dv) dv[slot] = sv[k];
      }
  }
  if (what == 0) {
    std::free(m->colptr); std::free(m->colind); std::free(m->colval);
    m->colptr = dp; m->colind = di; m->colval = dv;
  } else {
    std::free(m->rowptr); std::free(m->rowind); std::free(m->rowval);
    m->rowptr = dp; m->rowind = di; m->rowval = dv;
  }
}

slim_csr_t* model_from_columns(int32_t n, ssize_t* colptr, int32_t* colind,
                               float* colval, bool row_view) {
  slim_csr_t* m = csr_new();
  if (!m) return nullptr;
  m->nrows = m->ncols = n;
  m->colptr = colptr;
  m->colind = colind;
  m->colval = colval;
  if (row_view) csr_build_index(m, 1);
  return m;
}

// ---------------------------------------------------------------------------
// top-N (reference predict.c)
// ---------------------------------------------------------------------------
namespace {
// descending by score; equal scores keep their discovery order (the
// reference's gk_fkvsortd leaves tie order undefined)
int32_t emit_best(int32_t ncand, int32_t nrcmds, const std::vector<float>& key,
                  const std::vector<int32_t>& val, int32_t* rids, float* rscores) {
  std::vector<int32_t> order(ncand);
  std::iota(order.begin(), order.end(), 0);
  const int32_t n = std::min(ncand, nrcmds);
  auto better = [&](int32_t a, int32_t b) {
    return key[a] > key[b] || (key[a] == key[b] && a < b);
  };
  std::partial_sort(order.begin(), order.begin() + n, order.end(), better);
  for (int32_t r = 0; r < n; ++r) {
    rids[r] = val[order[r]];
    rscores[r] = key[order[r]];
  }
  return n;
}
}  // namespace

int32_t top_n(const slim_csr_t* W, int32_t nratings, const int32_t* itemids,
              const float* ratings, int32_t nrcmds, int32_t* rids, float* rscores,
              TopNScratch& ws) {
  const int32_t ncols = W->ncols, nrows = W->nrows;
  auto in_cols = [&](int32_t i) { return i >= 0 && i < ncols; };
  for (int32_t r = 0; r < nratings; ++r)
    if (in_cols(itemids[r])) ws.marker[itemids[r]] = -2;  // history: never recommended

  int32_t ncand = 0;
  for (int32_t r = 0; r < nratings; ++r) {
    const int32_t i = itemids[r];
    if (i < 0 || i >= nrows) continue;  // (the reference's guard cannot fire; ids
                                        //  outside the model are undefined there)
    const float rating = ratings ? ratings[r] : 1.0f;
    for (ssize_t j = W->rowptr[i]; j < W->rowptr[i + 1]; ++j) {
      const int32_t k = W->rowind[j];
      int32_t& slot = ws.marker[k];
      if (slot == -2) continue;
      if (slot == -1) {
        ws.val[ncand] = k;
        ws.key[ncand] = 0.0f;
        slot = ncand++;
      }
      ws.key[slot] += rating * W->rowval[j];
    }
  }
  const int32_t n = emit_best(ncand, nrcmds, ws.key, ws.val, rids, rscores);
  for (int32_t c = 0; c < ncand; ++c) ws.marker[ws.val[c]] = -1;
  for (int32_t r = 0; r < nratings; ++r)
    if (in_cols(itemids[r])) ws.marker[itemids[r]] = -1;
  return n;
}

// top_n is the yardstick the filtered scorers are tested against and stays as it is: this is its loop with the
// filter's marks.  The exclusion row is marked like the history (-2) before the walk; an id the bitmap does not
// allow is marked -2 when the walk first meets it (a user touches far fewer than ncols ids) and remembered, so
// that the marker leaves as it came: all -1.
int32_t top_n_filtered(const slim_csr_t* W, int32_t nratings, const int32_t* itemids,
                       const float* ratings, int32_t nrcmds, int32_t* rids, float* rscores,
                       TopNScratch& ws, const HostFilter& F, int32_t user) {
  const int32_t ncols = W->ncols, nrows = W->nrows;
  auto in_cols = [&](int32_t i) { return i >= 0 && i < ncols; };
  const int64_t x0 = F.xptr && user >= 0 && user < F.xusers ? F.xptr[user] : 0;
  const int64_t x1 = F.xptr && user >= 0 && user < F.xusers ? F.xptr[user + 1] : 0;
  for (int32_t r = 0; r < nratings; ++r)
    if (in_cols(itemids[r])) ws.marker[itemids[r]] = -2;  // history: never recommended
  for (int64_t x = x0; x < x1; ++x)
    if (in_cols(F.xind[x])) ws.marker[F.xind[x]] = -2;    // nor the user's exclusions

  int32_t ncand = 0;
  std::vector<int32_t> barred;  // ids the bitmap turned away
  for (int32_t r = 0; r < nratings; ++r) {
    const int32_t i = itemids[r];
    if (i < 0 || i >= nrows) continue;
    const float rating = ratings ? ratings[r] : 1.0f;
    for (ssize_t j = W->rowptr[i]; j < W->rowptr[i + 1]; ++j) {
      const int32_t k = W->rowind[j];
      int32_t& slot = ws.marker[k];
      if (slot == -2) continue;
      if (slot == -1) {
        if (F.bits && !((F.bits[k >> 5] >> (k & 31)) & 1u)) {
          slot = -2;
          barred.push_back(k);
          continue;
        }
        ws.val[ncand] = k;
        ws.key[ncand] = 0.0f;
        slot = ncand++;
      }
      ws.key[slot] += rating * W->rowval[j];
    }
  }
  const int32_t n = emit_best(ncand, nrcmds, ws.key, ws.val, rids, rscores);
  for (int32_t c = 0; c < ncand; ++c) ws.marker[ws.val[c]] = -1;
  for (const int32_t k : barred) ws.marker[k] = -1;
  for (int64_t x = x0; x < x1; ++x)
    if (in_cols(F.xind[x])) ws.marker[F.xind[x]] = -1;
  for (int32_t r = 0; r < nratings; ++r)
    if (in_cols(itemids[r])) ws.marker[itemids[r]] = -1;
  return n;
}

int32_t top_n_1vsk(const slim_csr_t* W, int32_t nratings, const int32_t* itemids,
                   const float* ratings, int32_t nrcmds, int32_t* rids,
                   float* rscores, int32_t nnegs, const int32_t* negitems) {
  const int32_t ncols = W->ncols, nrows = W->nrows;
  std::vector<int32_t> slot_of(ncols, -2);  // -2: not a candidate
  std::vector<float> key(nnegs, 0.0f);
  std::vector<int32_t> val(negitems, negitems + nnegs);
  for (int32_t c = 0; c < nnegs; ++c)
    if (negitems[c] >= 0 && negitems[c] < ncols) slot_of[negitems[c]] = c;
  for (int32_t r = 0; r < nratings; ++r) {
    const int32_t i = itemids[r];
    if (i < 0 || i >= nrows) continue;
    const float rating = ratings ? ratings[r] : 1.0f;
    for (ssize_t j = W->rowptr[i]; j < W->rowptr[i + 1]; ++j) {
      const int32_t s = slot_of[W->rowind[j]];
      if (s >= 0) key[s] += rating * W->rowval[j];
    }
  }
  return emit_best(nnegs, nrcmds, key, val, rids, rscores);
}

void score_candidates_host(const slim_csr_t* W, const slim_csr_t* trn, const HostCandSet& S, int32_t nrcmds,
                           float* slot_scores, int32_t* output, float* scores, int32_t* counts) {
  const int32_t ncols = W->ncols, nrows = W->nrows;
  std::vector<int32_t> slot_of(ncols, -2);  // -2: not a candidate
  std::vector<float> key;
  std::vector<int32_t> val;
  for (int32_t u = 0; u < trn->nrows; ++u) {
    const int32_t* cand = S.cind + S.cptr[u];
    const int32_t len = (int32_t)(S.cptr[u + 1] - S.cptr[u]);
    key.assign(len, 0.0f);
    val.assign(cand, cand + len);
    for (int32_t c = 0; c < len; ++c)
      if (cand[c] >= 0 && cand[c] < ncols) slot_of[cand[c]] = c;  // (a repeated id: the last occurrence)
    for (ssize_t h = trn->rowptr[u]; h < trn->rowptr[u + 1]; ++h) {
      const int32_t i = trn->rowind[h];
      if (i < 0 || i >= nrows) continue;
      const float rating = trn->rowval ? trn->rowval[h] : 1.0f;
      for (ssize_t j = W->rowptr[i]; j < W->rowptr[i + 1]; ++j) {
        const int32_t s = slot_of[W->rowind[j]];
        if (s >= 0) key[s] += rating * W->rowval[j];
      }
    }
    for (int32_t c = 0; c < len; ++c)
      if (cand[c] >= 0 && cand[c] < ncols) slot_of[cand[c]] = -2;
    if (slot_scores) std::copy(key.begin(), key.end(), slot_scores + S.cptr[u]);
    if (nrcmds > 0) {
      const int32_t n = emit_best(len, nrcmds, key, val, output + (ssize_t)u * nrcmds, scores + (ssize_t)u * nrcmds);
      if (counts) counts[u] = n;
    }
  }
}

void explain_candidates_host(const slim_csr_t* W, const slim_csr_t* trn, const HostCandSet& S, int32_t nwhy,
                             int32_t* why_items, float* why_terms, int32_t* support) {
  const int32_t ncols = W->ncols, nrows = W->nrows;
  std::vector<int32_t> slot_of(ncols, -2);  // -2: not a candidate
  std::vector<int32_t> count, item;         // per slot: its terms; its places, [slot][nwhy]
  std::vector<float> term;
  for (int32_t u = 0; u < trn->nrows; ++u) {
    const int32_t* cand = S.cind + S.cptr[u];
    const int32_t len = (int32_t)(S.cptr[u + 1] - S.cptr[u]);
    count.assign(len, 0);
    item.resize((size_t)len * nwhy);
    term.resize((size_t)len * nwhy);
    for (int32_t c = 0; c < len; ++c)
      if (cand[c] >= 0 && cand[c] < ncols) slot_of[cand[c]] = c;  // (a repeated id: the last occurrence)
    for (ssize_t h = trn->rowptr[u]; h < trn->rowptr[u + 1]; ++h) {
      const int32_t i = trn->rowind[h];
      if (i < 0 || i >= nrows) continue;
      const float rating = trn->rowval ? trn->rowval[h] : 1.0f;
      for (ssize_t j = W->rowptr[i]; j < W->rowptr[i + 1]; ++j) {
        const int32_t s = slot_of[W->rowind[j]];
        if (s < 0) continue;
        const float t = rating * W->rowval[j];
        // positions ascend, so among equal terms this one is the last: it goes in front of the first smaller one
        const int32_t have = std::min(count[s]++, nwhy);
        int32_t* si = item.data() + (size_t)s * nwhy;
        float* st = term.data() + (size_t)s * nwhy;
        int32_t k = have;
        while (k > 0 && st[k - 1] < t) --k;
        if (k >= nwhy) continue;
        for (int32_t m = std::min(have, nwhy - 1); m > k; --m) { si[m] = si[m - 1]; st[m] = st[m - 1]; }
        si[k] = i; st[k] = t;
      }
    }
    for (int32_t c = 0; c < len; ++c) {
      const int64_t e = S.cptr[u] + c;
      const bool live = cand[c] >= 0 && cand[c] < ncols && slot_of[cand[c]] == c;
      if (support) support[e] = live ? count[c] : 0;
      if (!live || !why_items) continue;
      const int32_t n = std::min(count[c], nwhy);
      std::copy(item.begin() + (size_t)c * nwhy, item.begin() + (size_t)c * nwhy + n, why_items + e * nwhy);
      std::copy(term.begin() + (size_t)c * nwhy, term.begin() + (size_t)c * nwhy + n, why_terms + e * nwhy);
    }
    for (int32_t c = 0; c < len; ++c)
      if (cand[c] >= 0 && cand[c] < ncols) slot_of[cand[c]] = -2;
  }
}

void sample_candidates_host(int32_t ncols, const slim_csr_t* trn, const slim_csr_t* tst, int32_t nusers,
                            const int32_t* users, int32_t nnegs, uint64_t seed, std::vector<int64_t>& cptr,
                            std::vector<int32_t>& cind, const uint64_t* wC) {
  const int32_t nall = std::min(trn->nrows, tst->nrows);
  const int32_t nsel = users ? nusers : nall;
  cptr.assign((size_t)nall + 1, 0);
  cind.clear();
  std::vector<uint8_t> mark((size_t)ncols, 0);  // X_u and the accepted ids; restored after each user
  std::vector<int32_t> marked;
  std::vector<std::pair<uint64_t, int32_t>> keyed;
  int32_t next = 0;  // rows [next, u) are empty
  for (int32_t q = 0; q < nsel; ++q) {
    const int32_t u = users ? users[q] : q;
    for (; next < u; ++next) cptr[(size_t)next + 1] = (int64_t)cind.size();
    next = u + 1;
    const ssize_t t0 = tst->rowptr[u], t1 = tst->rowptr[u + 1];
    if (t1 > t0) {
      marked.clear();
      auto put = [&](int32_t id) {
        if (id < 0 || id >= ncols || mark[id]) return;
        mark[id] = 1;
        marked.push_back(id);
      };
      for (ssize_t h = trn->rowptr[u]; h < trn->rowptr[u + 1]; ++h) put(trn->rowind[h]);
      for (ssize_t t = t0; t < t1; ++t) put(tst->rowind[t]);
      const int64_t E = (int64_t)marked.size();
      const uint64_t base = sample_base(seed, (uint64_t)u);
      if (wC) {
        // phase 1: draws from the full weights, rejecting what is taken; phase 2: over what is left, in id order
        const uint64_t T = wC[ncols];
        const int64_t stop = sample_guard(nnegs);
        int32_t got = 0;
        for (int64_t d = 0; d < stop && got < nnegs; ++d) {
          const int32_t id = sample_search(wC, ncols, sample_mulhi64(sample_key(base, (uint64_t)d), T));
          if (mark[id]) continue;
          mark[id] = 1;
          marked.push_back(id);
          cind.push_back(id);
          ++got;
        }
        if (got < nnegs) {
          uint64_t left = 0;  // the weights still in F
          for (int32_t i = 0; i < ncols; ++i)
            if (!mark[i]) left += wC[i + 1] - wC[i];
          for (int64_t j = 0; got < nnegs && left > 0; ++j) {
            const uint64_t r = sample_mulhi64(sample_key(base, (uint64_t)(stop + j)), left);
            uint64_t run = 0;
            int32_t id = 0;
            for (; id < ncols; ++id)
              if (!mark[id] && (run += wC[id + 1] - wC[id]) > r) break;
            mark[id] = 1;
            marked.push_back(id);
            cind.push_back(id);
            left -= wC[id + 1] - wC[id];
            ++got;
          }
        }
      } else if (2 * (E + nnegs) <= ncols) {
        int32_t got = 0;
        for (int64_t d = 0, stop = sample_guard(nnegs); d < stop && got < nnegs; ++d) {
          const int32_t id = (int32_t)sample_item(sample_key(base, (uint64_t)d), (uint32_t)ncols);
          if (mark[id]) continue;
          mark[id] = 1;
          marked.push_back(id);
          cind.push_back(id);
          ++got;
        }
      } else {
        keyed.clear();
        for (int32_t i = 0; i < ncols; ++i)
          if (!mark[i]) keyed.emplace_back(sample_key(base, (uint64_t)i), i);
        const size_t m = std::min<size_t>((size_t)nnegs, keyed.size());
        std::partial_sort(keyed.begin(), keyed.begin() + m, keyed.end());
        for (size_t k = 0; k < m; ++k) cind.push_back(keyed[k].second);
      }
      for (int32_t id : marked) mark[id] = 0;
      cind.insert(cind.end(), tst->rowind + t0, tst->rowind + t1);
    }
    cptr[(size_t)u + 1] = (int64_t)cind.size();
  }
  for (; next < nall; ++next) cptr[(size_t)next + 1] = (int64_t)cind.size();
}

int32_t* head_tail_split(int32_t nrows, int32_t ncols, const ssize_t* rowptr,
                         const int32_t* rowind) {
  std::vector<int64_t> pop(ncols, 0);
  for (ssize_t k = 0; k < rowptr[nrows]; ++k)
    if (rowind[k] >= 0 && rowind[k] < ncols) ++pop[rowind[k]];
  return head_tail_from_counts(ncols, pop, rowptr[nrows]);
}

int32_t* head_tail_from_counts(int32_t ncols, const std::vector<int64_t>& pop, int64_t nnz) {
  int32_t* mark = xmalloc<int32_t>(ncols);
  std::vector<int32_t> by_pop(ncols);
  std::iota(by_pop.begin(), by_pop.end(), 0);
  std::stable_sort(by_pop.begin(), by_pop.end(),
                   [&](int32_t a, int32_t b) { return pop[a] > pop[b]; });
  std::fill(mark, mark + ncols, 1);
  int64_t budget = nnz / 2;
  for (int32_t c = 0; c < ncols && budget > 0; ++c) {
    mark[by_pop[c]] = 0;
    budget -= pop[by_pop[c]];
  }
  return mark;
}

EvalResult evaluate(const slim_csr_t* model, const slim_csr_t* trn,
                    const slim_csr_t* tst, int32_t nrcmds, const int32_t* fmarker,
                    int32_t fm_ncols, const int32_t* lists, const int32_t* counts) {
  EvalResult out;
  TopNScratch ws(std::max(model->ncols, model->nrows));
  std::vector<int32_t> rids(nrcmds);
  std::vector<float> rsc(nrcmds);
  std::vector<int32_t> wanted(std::max(fm_ncols, model->ncols), -1);
  // accumulators are float in the reference (pyapi.c:223-230)
  float hr_all = 0, hr_head = 0, hr_tail = 0, arhr = 0;
  const int32_t nusers = std::min(trn->nrows, tst->nrows);
  for (int32_t u = 0; u < nusers; ++u) {
    const ssize_t t0 = tst->rowptr[u], t1 = tst->rowptr[u + 1];
    if (t1 - t0 < 1) continue;
    const ssize_t h0 = trn->rowptr[u], h1 = trn->rowptr[u + 1];
    int32_t n;
    if (lists) {
      n = counts[u];
      std::copy(lists + (size_t)u * nrcmds, lists + (size_t)u * nrcmds + n, rids.begin());
    } else {
      n = top_n(model, int32_t(h1 - h0), trn->rowind + h0,
                trn->rowval ? trn->rowval + h0 : nullptr, nrcmds, rids.data(), rsc.data(), ws);
    }
    ++out.nvalid;
    int32_t ntrue[2] = {0, 0}, nhits[3] = {0, 0, 0};
    bool has_head = false, has_tail = false;
    float gain = 0, ideal = 0;
    for (ssize_t z = t0; z < t1; ++z) {
      const int32_t it = tst->rowind[z];
      wanted[it] = u;
      ++ntrue[fmarker[it]];
      (fmarker[it] ? has_tail : has_head) = true;
      ideal += 1.0 / (1.0 + double(z - t0));
    }
    out.nvalid_head += has_head;
    out.nvalid_tail += has_tail;
    for (int32_t r = 0; r < n; ++r)
      if (wanted[rids[r]] == u) {
        ++nhits[fmarker[rids[r]]];
        ++nhits[2];
        gain += 1.0 / (1.0 + r);
      }
    hr_head += nhits[0] > 0 ? 1.0 * nhits[0] / ntrue[0] : 0.0;
    hr_tail += nhits[1] > 0 ? 1.0 * nhits[1] / ntrue[1] : 0.0;
    hr_all += 1.0 * nhits[2] / double(t1 - t0);
    arhr += gain / ideal;
  }
  out.hr = out.nvalid > 0 ? hr_all / out.nvalid : 0;
  out.hr_head = out.nvalid_head > 0 ? hr_head / out.nvalid_head : 0;
  out.hr_tail = out.nvalid_tail > 0 ? hr_tail / out.nvalid_tail : 0;
  out.arhr = out.nvalid > 0 ? arhr / out.nvalid : 0;
  return out;
}

// ---------------------------------------------------------------------------
// files
// ---------------------------------------------------------------------------
bool write_binrow(const slim_csr_t* m, const char* path) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  const int64_t nnz = m->rowptr[m->nrows];
  bool ok = std::fwrite(&m->nrows, sizeof(int32_t), 1, f) == 1 &&
            std::fwrite(&m->ncols, sizeof(int32_t), 1, f) == 1 &&
            std::fwrite(m->rowptr, sizeof(ssize_t), m->nrows + 1, f) == size_t(m->nrows + 1) &&
            std::fwrite(m->rowind, sizeof(int32_t), nnz, f) == size_t(nnz) &&
            (!m->rowval || std::fwrite(m->rowval, sizeof(float), nnz, f) == size_t(nnz));
  return std::fclose(f) == 0 && ok;
}

slim_csr_t* read_binrow(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return nullptr;
  slim_csr_t* m = csr_new();
  bool ok = std::fread(&m->nrows, sizeof(int32_t), 1, f) == 1 &&
            std::fread(&m->ncols, sizeof(int32_t), 1, f) == 1 && m->nrows >= 0;
  if (ok) {
    m->rowptr = xmalloc<ssize_t>(m->nrows + 1);
    ok = std::fread(m->rowptr, sizeof(ssize_t), m->nrows + 1, f) == size_t(m->nrows + 1);
  }
  if (ok) {
    const int64_t nnz = m->rowptr[m->nrows];
    m->rowind = xmalloc<int32_t>(nnz);
    m->rowval = xmalloc<float>(nnz);
    ok = std::fread(m->rowind, sizeof(int32_t), nnz, f) == size_t(nnz) &&
         std::fread(m->rowval, sizeof(float), nnz, f) == size_t(nnz);
  }
  std::fclose(f);
  if (!ok) {
    csr_free(m);
    return nullptr;
  }
  return m;
}

bool write_text_csr(const slim_csr_t* m, const char* path) {
  FILE* f = std::fopen(path, "w");
  if (!f) return false;
  for (int32_t r = 0; r < m->nrows; ++r) {
    for (ssize_t k = m->rowptr[r]; k < m->rowptr[r + 1]; ++k) {
      // %.9g round-trips a float exactly; GKlib's writer prints fewer digits,
      // any float syntax is accepted by both readers
      if (m->rowval) std::fprintf(f, " %d %.9g", m->rowind[k], double(m->rowval[k]));
      else std::fprintf(f, " %d", m->rowind[k]);
    }
    std::fputc('\n', f);
  }
  return std::fclose(f) == 0;
}

slim_csr_t* read_text_csr(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return nullptr;
  std::vector<ssize_t> ptr{0};
  std::vector<int32_t> ind;
  std::vector<float> val;
  char* line = nullptr;
  size_t cap = 0;
  bool ok = true;
  while (getline(&line, &cap, f) >= 0) {
    char* p = line;
    for (;;) {
      char* e;
      const long id = std::strtol(p, &e, 10);
      if (e == p) break;
      p = e;
      const float v = std::strtof(p, &e);
      if (e == p) { ok = false; break; }  // id without a value
      p = e;
      ind.push_back(int32_t(id));
      val.push_back(v);
    }
    ptr.push_back(ssize_t(ind.size()));
  }
  std::free(line);
  std::fclose(f);
  if (!ok) return nullptr;
  slim_csr_t* m = csr_from_rows(int32_t(ptr.size() - 1), ptr.data(), ind.data(), val.data());
  return m;
}

// ---- slim_gpu_exposure.h ------------------------------------------------------
int32_t exposure_cutoffs_check(const char* who, int32_t nrcmds, int32_t ncutoffs, const int32_t* cutoffs) {
  std::string what;
  if (nrcmds < 1) what = "nrcmds must be at least 1, not " + std::to_string(nrcmds);
  else if (!cutoffs || ncutoffs < 1 || ncutoffs > SLIMGPU_MAX_CUTOFFS)
    what = "between 1 and " + std::to_string(SLIMGPU_MAX_CUTOFFS) + " cutoffs, not " + std::to_string(ncutoffs);
  for (int32_t k = 0; k < ncutoffs && what.empty(); ++k) {
    if (cutoffs[k] < 1) what = "a cutoff must be at least 1, not " + std::to_string(cutoffs[k]);
    else if (k > 0 && cutoffs[k] <= cutoffs[k - 1]) what = "the cutoffs must ascend strictly";
  }
  if (what.empty() && cutoffs[ncutoffs - 1] > nrcmds)
    what = "the last cutoff is " + std::to_string(cutoffs[ncutoffs - 1]) + ", the lists have " +
           std::to_string(nrcmds) + " places";
  if (what.empty()) return SLIM_OK;
  set_error(std::string(who) + ": " + what);
  return SLIM_ERROR_INPUT;
}

int32_t exposure_lists_check(const char* who, int32_t ncols, int64_t nlists, int32_t nrcmds, const int32_t* ids,
                             const int32_t* counts, int32_t ncutoffs, const int32_t* cutoffs) {
  if (const int32_t rc = exposure_cutoffs_check(who, nrcmds, ncutoffs, cutoffs); rc != SLIM_OK) return rc;
  std::string what;
  if (ncols < 1) what = "ncols must be at least 1, not " + std::to_string(ncols);
  else if (nlists < 0) what = "nlists must be at least 0, not " + std::to_string(nlists);
  else if (nlists > 0 && !ids) what = "no lists are given for nlists = " + std::to_string(nlists);
  for (int64_t q = 0; counts && q < nlists && what.empty(); ++q)
    if (counts[q] < 0 || counts[q] > nrcmds)
      what = "counts[" + std::to_string(q) + "] is " + std::to_string(counts[q]) + ", outside [0, " +
             std::to_string(nrcmds) + "]";
  if (what.empty()) return SLIM_OK;
  set_error(std::string(who) + ": " + what);
  return SLIM_ERROR_INPUT;
}

void list_exposure_host(int32_t ncols, int64_t nlists, int32_t nrcmds, const int32_t* ids, const int32_t* counts,
                        int32_t K, const int32_t* cutoffs, uint32_t* E, int64_t* outside) {
  std::fill(E, E + (size_t)K * (size_t)ncols, 0u);
  std::fill(outside, outside + K, (int64_t)0);
  for (int64_t q = 0; q < nlists; ++q) {
    const int32_t len = std::min(counts ? counts[q] : nrcmds, cutoffs[K - 1]);
    const int32_t* row = ids + q * (int64_t)nrcmds;
    int32_t b = 0;  // the band of place p: the first cutoff above it
    for (int32_t p = 0; p < len; ++p) {
      while (p >= cutoffs[b]) ++b;
      const int32_t i = row[p];
      if (i < 0 || i >= ncols) ++outside[b];
      else ++E[(size_t)b * (size_t)ncols + (size_t)i];
    }
  }
  for (int32_t k = 1; k < K; ++k) {
    outside[k] += outside[k - 1];
    for (int32_t i = 0; i < ncols; ++i) E[(size_t)k * (size_t)ncols + i] += E[(size_t)(k - 1) * (size_t)ncols + i];
  }
}

void exposure_summary(int32_t ncols, const uint32_t* pop, const int32_t* fmarker, int32_t fm_ncols, int64_t nlists,
                      const uint32_t* E, int64_t outside, slimgpu_exposure_t* out) {
  typedef __int128 wide;
  slimgpu_exposure_t s = {};
  s.lists = nlists; s.outside = outside; s.ncols = ncols;
  wide popsum = 0;
  for (int32_t i = 0; i < ncols; ++i) {
    const uint32_t e = E[i];
    if (!e) continue;
    s.slots += e;
    ++s.distinct;
    if (fmarker && (i >= fm_ncols || fmarker[i] != 0)) s.tail_slots += e;
    if (pop) popsum += (wide)e * (wide)pop[i];
  }
  std::vector<uint32_t> x(E, E + ncols);
  std::sort(x.begin(), x.end());
  wide gnum = 0;
  for (int32_t j = 1; j <= ncols; ++j) gnum += (wide)(2 * (int64_t)j - ncols - 1) * (wide)x[(size_t)j - 1];
  auto ratio = [](wide num, wide den) { return den == 0 ? 0.0 : (double)num / (double)den; };
  s.coverage = ratio(s.distinct, ncols);
  s.tail_share = ratio(s.tail_slots, s.slots);
  s.gini = ratio(gnum, (wide)ncols * (wide)s.slots);
  s.avg_pop = ratio(popsum, s.slots);
  *out = s;
}

int32_t group_partition(const char* who, int32_t nsel, const int32_t* users, int32_t nall, int32_t ngroups,
                        const int32_t* group_of_user, int32_t* order, int64_t* offsets) {
  std::string what;
  if (ngroups < 1 || ngroups > SLIMGPU_MAX_GROUPS)
    what = "between 1 and " + std::to_string(SLIMGPU_MAX_GROUPS) + " groups, not " + std::to_string(ngroups);
  else if (nsel < 0 || nall < 0 || !offsets || (nall > 0 && !group_of_user) || (nsel > 0 && !order))
    what = "bad arguments (a group for every user, the order and the offsets)";
  else if (!users && nsel > nall)
    what = std::to_string(nsel) + " positions and " + std::to_string(nall) + " users";
  for (int32_t u = 0; u < nall && what.empty(); ++u)
    if (group_of_user[u] < -1 || group_of_user[u] >= ngroups)
      what = "user " + std::to_string(u) + " has group " + std::to_string(group_of_user[u]) + ", outside [-1, " +
             std::to_string(ngroups) + ")";
  for (int32_t q = 0; users && q < nsel && what.empty(); ++q)
    if (users[q] < 0 || users[q] >= nall)
      what = "user " + std::to_string(users[q]) + " is outside [0, " + std::to_string(nall) + ")";
  if (!what.empty()) {
    set_error(std::string(who) + ": " + what);
    return SLIM_ERROR_INPUT;
  }
  // a stable counting sort: the members of every group, then their places in position order
  std::fill(offsets, offsets + ngroups + 1, (int64_t)0);
  for (int32_t q = 0; q < nsel; ++q) {
    const int32_t g = group_of_user[users ? users[q] : q];
    if (g >= 0) ++offsets[g + 1];
  }
  for (int32_t g = 0; g < ngroups; ++g) offsets[g + 1] += offsets[g];
  std::vector<int64_t> next(offsets, offsets + ngroups);
  for (int32_t q = 0; q < nsel; ++q) {
    const int32_t g = group_of_user[users ? users[q] : q];
    if (g >= 0) order[next[(size_t)g]++] = q;
  }
  return SLIM_OK;
}

// ---- slim_gpu_split.h ---------------------------------------------------------
int32_t split_check(const char* who, const slimgpu_split_t* s) {
  std::string what;
  if (!s) {
    what = "bad arguments (the split's parameters)";
  } else {
    const bool leave = s->mode == SLIMGPU_SPLIT_LEAVE_OUT, folds = s->mode == SLIMGPU_SPLIT_FOLDS;
    if (!leave && !folds)
      what = "mode must be SLIMGPU_SPLIT_LEAVE_OUT (0) or SLIMGPU_SPLIT_FOLDS (1), not " + std::to_string(s->mode);
    else if (s->nfolds < (folds ? 2 : 1))
      what = std::string("nfolds must be at least ") + (folds ? "2 in folds mode" : "1") + ", not " +
             std::to_string(s->nfolds);
    else if (s->fold < 0 || s->fold >= s->nfolds)
      what = "fold " + std::to_string(s->fold) + " is outside [0, " + std::to_string(s->nfolds) + ")";
    else if (s->minkeep < 1)
      what = "minkeep must be at least 1, not " + std::to_string(s->minkeep);
    else if (leave && s->nheld < 1)
      what = "nheld must be at least 1, not " + std::to_string(s->nheld);
    else if (leave && (int64_t)s->nfolds * s->nheld > SLIMGPU_SPLIT_MAX_HELD)
      what = "nfolds * nheld is " + std::to_string((int64_t)s->nfolds * s->nheld) + ", above " +
             std::to_string(SLIMGPU_SPLIT_MAX_HELD) + ": the selection keeps that many smallest keys per row";
  }
  if (what.empty()) return SLIM_OK;
  set_error(std::string(who) + ": " + what);
  return SLIM_ERROR_INPUT;
}

int32_t split_host(const slim_csr_t* data, const slimgpu_split_t& s, slim_csr_t** trn, slim_csr_t** tst) {
  const int32_t nrows = data->nrows;
  const ssize_t* ptr = data->rowptr;
  const int32_t* ind = data->rowind;
  const float* val = data->rowval;
  const int64_t nnz = ptr[nrows];
  for (int64_t k = 0; k < nnz; ++k)
    if (ind[k] < 0) {
      set_error("SLIMGPU_SplitHost: entry " + std::to_string(k) + " has item id " + std::to_string(ind[k]) +
                ", below 0");
      return SLIM_ERROR_INPUT;
    }
  const bool leave = s.mode == SLIMGPU_SPLIT_LEAVE_OUT;
  const uint64_t F = (uint64_t)s.nfolds, f = (uint64_t)s.fold;
  const int64_t h = s.nheld, m = s.minkeep;
  std::vector<uint8_t> held((size_t)nnz, 0);
  std::vector<ssize_t> tptr((size_t)nrows + 1, 0);
  struct Rec {
    uint64_t key;
    int32_t item;
    int64_t pos;
    bool operator<(const Rec& o) const {
      return key != o.key ? key < o.key : item != o.item ? item < o.item : pos < o.pos;
    }
  };
  std::vector<Rec> recs;
  for (int32_t u = 0; u < nrows; ++u) {
    const int64_t r0 = ptr[u], L = ptr[u + 1] - r0;
    const uint64_t base = sample_base(s.seed, (uint64_t)u);
    int64_t out = 0;
    if (leave) {
      if (L >= (int64_t)F * h + m) {
        recs.clear();
        for (int64_t p = 0; p < L; ++p) recs.push_back({sample_key(base, (uint64_t)ind[r0 + p]), ind[r0 + p], p});
        const int64_t lo = (int64_t)f * h, hi = lo + h;  // ranks [lo, hi)
        std::partial_sort(recs.begin(), recs.begin() + hi, recs.end());
        for (int64_t r = lo; r < hi; ++r) held[(size_t)(r0 + recs[(size_t)r].pos)] = 1;
        out = h;
      }
    } else {
      int64_t inside = 0;
      for (int64_t p = 0; p < L; ++p)
        inside += sample_mulhi64(sample_key(base, (uint64_t)ind[r0 + p]), F) == f;
      if (inside >= 1 && L - inside >= m) {
        for (int64_t p = 0; p < L; ++p)
          held[(size_t)(r0 + p)] = sample_mulhi64(sample_key(base, (uint64_t)ind[r0 + p]), F) == f;
        out = inside;
      }
    }
    tptr[(size_t)u + 1] = tptr[(size_t)u] + out;
  }
  const int64_t nt = tptr[(size_t)nrows], nk = nnz - nt;
  slim_csr_t* halves[2] = {csr_new(), csr_new()};  // train, test
  bool ok = halves[0] && halves[1];
  for (int w = 0; w < 2 && ok; ++w) {
    slim_csr_t* o = halves[w];
    const int64_t n = w ? nt : nk;
    o->nrows = nrows;
    o->rowptr = xmalloc<ssize_t>((size_t)nrows + 1);
    o->rowind = xmalloc<int32_t>((size_t)n);
    o->rowval = val ? xmalloc<float>((size_t)n) : nullptr;
    ok = o->rowptr && o->rowind && (!val || o->rowval);
  }
  if (!ok) {
    csr_free(halves[0]);
    csr_free(halves[1]);
    set_error("SLIMGPU_SplitHost: out of host memory");
    return SLIM_ERROR_MEMORY;
  }
  int64_t at[2] = {0, 0};
  for (int32_t u = 0; u < nrows; ++u) {
    halves[0]->rowptr[u] = at[0];
    halves[1]->rowptr[u] = at[1];
    for (int64_t k = ptr[u]; k < ptr[u + 1]; ++k) {
      const int w = held[(size_t)k];
      halves[w]->rowind[at[w]] = ind[k];
      if (val) halves[w]->rowval[at[w]] = val[k];
      ++at[w];
    }
  }
  for (int w = 0; w < 2; ++w) {
    halves[w]->rowptr[nrows] = at[w];
    halves[w]->ncols = max_index_plus_one(at[w], halves[w]->rowind);
  }
  *trn = halves[0];
  *tst = halves[1];
  return SLIM_OK;
}

}  // namespace slimamd

extern "C" int32_t SLIMGPU_SplitHost(slim_t* data, const slimgpu_split_t* split, slim_t** trn, slim_t** tst) {
  using namespace slimamd;
  set_error("");
  const slim_csr_t* d = static_cast<const slim_csr_t*>(data);
  if (!d || !d->rowptr || d->nrows < 0 || (d->rowptr[d->nrows] > 0 && !d->rowind) || !trn || !tst) {
    set_error("SLIMGPU_SplitHost: bad arguments (a matrix with a row view, the two outputs)");
    return SLIM_ERROR_INPUT;
  }
  if (const int32_t rc = split_check("SLIMGPU_SplitHost", split); rc != SLIM_OK) return rc;
  slim_csr_t *a = nullptr, *b = nullptr;
  try {
    const int32_t rc = split_host(d, *split, &a, &b);
    if (rc != SLIM_OK) return rc;
  } catch (const std::bad_alloc&) {
    set_error("SLIMGPU_SplitHost: out of host memory");
    return SLIM_ERROR_MEMORY;
  }
  *trn = a;
  *tst = b;
  return SLIM_OK;
}
