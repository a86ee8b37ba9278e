// Requests of the path kernels (path_kernels.hpp: marginals, loop-closure gate) -> rounds of device records.  Pure host code, no HIP: the
// round driver of sslam_chol.hip uploads what path_round made, and a stand-alone host program can include this header (tests/path_rounds_check.cpp).
//
// THE RULES, each written here and nowhere else:
//   * the path of an unknown is its column (h_xoff_col) and that column's ancestors (h_cparent) up to the root of the elimination tree;
//   * a record is `width` ints: v[0] first entry of path(u) in the round's path columns, v[1] its length, v[2], v[3] the same for path(v),
//     v[4] d(u), v[5] d(v), v[6] length of the common suffix of the two paths, v[7] scratch slice in units of 16 bytes (0: LDS),
//     v[8..] the caller's payload, untouched;
//   * fold (marginals): xoff_v == xoff_u is ONE path: v[2] = v[0], v[3] = 0, v[5] = d(u), v[6] = v[1];
//   * no_column (gate): an end with xoff < 0 has a path of length 0; without it such an end is an error, as is any unknown that is not the
//     start of a block row;
//   * a request of ylen = v[1] + v[3] path entries runs out of scratch iff fixed + ylen * kPathEntry + 16 > budget; its slice is
//     ylen * kPathEntry bytes rounded up to 16;
//   * a round always takes its first request, and goes on while it holds fewer than path_cap path ints and fewer than scratch_cap scratch
//     bytes: the caps are tested BEFORE a request is added, a round may overshoot either by one request;
//   * within a round the records are [LDS | scratch], each group in request order; src[i] is the request of record i.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace sslam {

constexpr size_t kPathEntry = 36 * sizeof(double) + 4 * sizeof(int) + sizeof(int);   // Y block, path record (int4), y offset of one path entry: 308

// A request is width - 4 ints: {xoff_u, dim_u, xoff_v, dim_v} -- first unknown (internal row order) and dimension of either end -- then
// the width - 8 payload ints (MarginalReq and GateReq of graph_engine.hpp are these ints).
struct PathRules {
  int width;            // ints per record: 8 (marginals) or 12 (gate)
  size_t fixed;         // bytes of the kernel's fixed LDS area
  size_t budget;        // LDS bytes a workgroup may take
  bool no_column;       // xoff < 0: path of length 0 (else: refused)
  bool fold;            // xoff_v == xoff_u: one path, nc = Pu
  size_t path_cap, scratch_cap;
};

struct PathRound {
  std::vector<int> up;        // [records: m x width | path columns]: what the kernels read
  std::vector<size_t> src;    // request of every record
  int m = 0, n_lds = 0, ylen_lds = 0;
  size_t scr_bytes = 0;
  size_t next = 0;            // first request of the next round
};

inline int path_col_of(const std::vector<int>& h_xoff_col, int xo) { return (xo >= 0 && xo < (int)h_xoff_col.size()) ? h_xoff_col[xo] : -1; }

// every end names a column (or, no_column, none at all)
inline bool path_reqs_valid(const std::vector<int>& h_xoff_col, const int* reqs, size_t n, int width, bool no_column) {
  for (size_t k = 0; k < n; ++k)
    for (int xo : {reqs[k * (width - 4)], reqs[k * (width - 4) + 2]})
      if (!(no_column && xo < 0) && path_col_of(h_xoff_col, xo) < 0) return false;
  return true;
}

// The round that starts at request k0 of n.  The vectors of R are reused from round to round.
inline void path_round(const std::vector<int>& h_xoff_col, const std::vector<int>& h_cparent, const int* reqs, size_t n, size_t k0,
                       const PathRules& rules, PathRound& R) {
  const int W = rules.width;
  std::vector<int> recs, cols;   // records in request order
  std::vector<char> scratch;
  R.n_lds = 0; R.ylen_lds = 0; R.scr_bytes = 0;
  size_t k = k0;
  for (; k < n && (k == k0 || (cols.size() < rules.path_cap && R.scr_bytes < rules.scratch_cap)); ++k) {
    const int* rq = reqs + k * (W - 4);
    const int xoff_u = rq[0], dim_u = rq[1], xoff_v = rq[2], dim_v = rq[3];
    recs.resize(recs.size() + W, 0);
    int* v = recs.data() + recs.size() - W;
    auto walk = [&](int xo, int& first, int& len) {
      first = (int)cols.size();
      for (int j = path_col_of(h_xoff_col, xo); j >= 0; j = h_cparent[j]) cols.push_back(j);
      len = (int)cols.size() - first;
    };
    walk(xoff_u, v[0], v[1]);
    v[4] = dim_u;
    if (rules.fold && xoff_v == xoff_u) { v[2] = v[0]; v[3] = 0; v[5] = dim_u; v[6] = v[1]; }
    else {
      walk(xoff_v, v[2], v[3]);
      v[5] = dim_v;
      int nc = 0;   // common suffix of the two paths: from the root down to their lowest common ancestor (none when an end has no column)
      while (nc < v[1] && nc < v[3] && cols[v[0] + v[1] - 1 - nc] == cols[v[2] + v[3] - 1 - nc]) ++nc;
      v[6] = nc;
    }
    std::copy(rq + 4, rq + W - 4, v + 8);
    const int ylen = v[1] + v[3];
    const bool scr = rules.fixed + (size_t)ylen * kPathEntry + 16 > rules.budget;
    if (scr) { v[7] = (int)(R.scr_bytes / 16); R.scr_bytes += ((size_t)ylen * kPathEntry + 15) & ~(size_t)15; }
    else { R.ylen_lds = std::max(R.ylen_lds, ylen); ++R.n_lds; }
    scratch.push_back(scr);
  }
  R.m = (int)(k - k0);
  R.next = k;
  R.up.resize((size_t)R.m * W + cols.size());
  R.src.resize(R.m);
  int at[2] = {0, R.n_lds};   // [LDS records | scratch records], request order within each
  for (int i = 0; i < R.m; ++i) {
    const int to = at[(int)scratch[i]]++;
    std::copy(recs.begin() + (size_t)i * W, recs.begin() + (size_t)(i + 1) * W, R.up.begin() + (size_t)to * W);
    R.src[to] = k0 + i;
  }
  std::copy(cols.begin(), cols.end(), R.up.begin() + (size_t)R.m * W);
}

}  // namespace sslam
