// Host graphs -> the tables of a device batch (g2o initializeOptimization + BlockSolver::buildStructure analogue; symbolic work only).
// Pure host code, no HIP: batch_upload (sslam_graph.hip) sends what batch_compile made, the plan introspection (sslam_debug_plan_*) serves
// the same tables to CPU tests, and a stand-alone host program can include this header.
//
// THE ORDER CONTRACT.  The linearisation kernels sum an unknown's contributions in the order of these tables, so the orders below decide the
// bits of H, b and everything computed from them:
//   * class arrays are ordered by graph, then by edge id;
//   * unique blocks (ppoff, plblk, llblk) are numbered by first appearance in class order;
//   * the block code of an EdgeSE3 is index * 2 + (row_i > row_j), of a landmark / point-point edge the index; -1: an end is not a row;
//   * the first edge on a row pair owns the block, later ones are coded -2 - code and listed in dup_eo / dup_el, stable-sorted by block;
//   * the slots of a pose row are all its EdgeSE3 ends in edge order, then its landmark edges in edge order;
//   * landmark-row slots, point-point slots, the edges of a landmark-landmark block and the priors of a pose row are in edge order;
//   * prow_perm is a stable sort within each graph by (EdgeSE3 slot count, total slot count);
//   * adj rows are sorted by column offset;
//   * H = Hpp_diag | Hll_diag | (pad to even) Hpp_off | Hpl | Hll_off: hpp_off_base is even, and b sits right behind H (batch_upload).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <unordered_map>
#include <utility>
#include <vector>
#include "graph_host.hpp"

namespace sslam {

// One storage class (EC_*) of edges: ends, block code, origin and SoA payload of every edge.
struct EdgeClassTab {
  std::vector<int> a, b;   // global index of each end in the pose / landmark arrays (b = -1: unary)
  std::vector<int> blk;    // off-diagonal block code (see the contract), -1: none
  std::vector<int> id, g;  // graph-local edge id, owning graph
  std::vector<int> dim;    // error dimension of the edge's type (a class may hold narrower types than its payload)
  std::vector<double> z, w;   // SoA: z[class_nz][n], upper triangle of Omega [upper_len(class_d)][n]
  int n() const { return (int)id.size(); }
};

// The part of the tables the host still reads once they are on the device (a Batch keeps it): index maps, unique blocks, the layout of H.
struct BatchMaps {
  std::vector<GraphSeg> seg;
  std::vector<std::vector<int>> v2pose, v2lm;   // per graph: vertex id -> global pose / landmark index, -1
  std::vector<int> pose_row, lm_row;            // global pose / landmark index -> row, -1: fixed or without an edge
  std::vector<int> prow_pose, lrow_lm;          // row -> global pose / landmark index
  std::vector<int> pose_vertex, lm_vertex;      // global pose / landmark index -> vertex id in its graph
  std::vector<std::pair<int, int>> ppoff;   // unique pose-pose blocks (row a < row b)
  std::vector<std::pair<int, int>> plblk;   // unique pose-landmark blocks (pose row, landmark row)
  std::vector<std::pair<int, int>> llblk;   // unique landmark-landmark blocks (row a < row b): point-point edges
  int64_t hll_base = 0, hpp_off_base = 0, hpl_base = 0, hll_off_base = 0, h_total = 0;   // layout of H, in doubles
  bool has_planes = false;
  int nPr() const { return (int)prow_pose.size(); }
  int nLr() const { return (int)lrow_lm.size(); }
};

struct BatchTables : BatchMaps {
  std::vector<int> prow_graph, lrow_graph;
  std::vector<unsigned char> lm_kind;           // VT_POINT / VT_PLANE
  // thread -> row of the pose-row kernel: within a graph, rows with the same numbers of EdgeSE3 and landmark slots next to each other.  The
  // lanes of a wave walk their rows' slots in step; a chain pose has two EdgeSE3 slots, the ~200 endpoints of the loop closures of an L
  // graph three or four, and spread over the graph's 78 waves they made nearly every wave run the EdgeSE3 arithmetic a third and fourth
  // time for one or two lanes.  Sorted, those rows fill three waves of their own (2.07 -> 2.02 ms per 512-graph build).
  std::vector<int> prow_perm;
  EdgeClassTab cls[kEdgeClasses];
  std::vector<int> dup_eo, dup_el;          // non-owner edges of shared blocks
  std::vector<int> pslot_ptr, lslot_ptr, llslot_ptr, llblk_ptr;   // CSRs over pose rows, landmark rows (twice), landmark-landmark blocks
  std::vector<std::array<int, 4>> pslot_rec;    // {edge, kind (0: EdgeSE3 seen from its i side, 1: from its j side, 2: landmark edge), end a, end b}
  std::vector<int> lslot_edge, llblk_edge;
  std::vector<std::array<int, 2>> llslot_rec;   // {point-point edge, side (0: first vertex, 1: second)}
  std::vector<int> ep_row, ep_ptr, ep_edge;     // pose rows that carry priors and a CSR over THEM (a prior on a fixed pose adds to chi2 only)
  std::vector<int> adj_ptr, adj_blk, adj_x;     // row adjacency for SpMV (pose rows, then landmark rows): offset of the block in H, of the column in x
  std::vector<unsigned char> adj_fmt;
  std::vector<int> shard_lo, shard_hi;          // edge-sharded mode: every graph's id range of this rank (all edges until sslam_batch_set_edge_shard)
  int max_row_chunks = 1, max_edge_chunks = 1;
};

// Unique (row, row) pairs numbered by first appearance.
struct BlockIndex {
  std::vector<std::pair<int, int>>& list;
  std::unordered_map<uint64_t, int> map;
  int find_or_add(int a, int c) {
    const auto ins = map.emplace(((uint64_t)(uint32_t)a << 32) | (uint32_t)c, (int)list.size());
    if (ins.second) list.push_back({a, c});
    return ins.first->second;
  }
};

// The first edge with a block code owns the block; a later one is coded -2 - code and listed in dup, stable-sorted by block.  shift: the low
// bits of a code that are not part of the block index (the swap bit of an EdgeSE3).
inline void code_duplicates(std::vector<int>& blk, int shift, size_t nblocks, std::vector<int>& dup) {
  std::vector<char> seen(nblocks, 0);
  dup.clear();
  for (int k = 0; k < (int)blk.size(); ++k) {
    if (blk[k] < 0) continue;
    if (seen[blk[k] >> shift]) { dup.push_back(k); blk[k] = -2 - blk[k]; }
    else seen[blk[k] >> shift] = 1;
  }
  std::stable_sort(dup.begin(), dup.end(), [&](int x, int y) { return ((-2 - blk[x]) >> shift) < ((-2 - blk[y]) >> shift); });
}

// List of lists -> CSR, items in list order.  With `kept`, empty rows are left out and the rows that stay are recorded there.
template <class T, class U, class F>
inline void lists_to_csr(const std::vector<std::vector<T>>& rows, std::vector<int>& ptr, std::vector<U>& items, F conv, std::vector<int>* kept = nullptr) {
  ptr.assign(1, 0);
  items.clear();
  for (size_t r = 0; r < rows.size(); ++r) {
    if (kept) { if (rows[r].empty()) continue; kept->push_back((int)r); }
    for (const T& x : rows[r]) items.push_back(conv(x));
    ptr.push_back((int)items.size());
  }
}

inline BatchTables batch_compile(const std::vector<HostGraph*>& graphs) {
  BatchTables T;
  const int B = (int)graphs.size();
  T.seg.assign(B, GraphSeg{});
  T.v2pose.assign(B, {}); T.v2lm.assign(B, {});
  T.shard_lo.assign(B, 0); T.shard_hi.assign(B, 0x7fffffff);
  EdgeClassTab& EO = T.cls[EC_SE3]; EdgeClassTab& EL = T.cls[EC_LANDMARK]; EdgeClassTab& ELL = T.cls[EC_POINT_POINT]; EdgeClassTab& EP = T.cls[EC_PRIOR];
  // ---- vertices -> pose / landmark indices and rows; edges -> their classes
  for (int g = 0; g < B; ++g) {
    const HostGraph& G = *graphs[g];
    std::vector<int> hidx;
    hessian_indices(G, hidx);
    GraphSeg& sg = T.seg[g];
    sg.pose0 = (int)T.pose_row.size(); sg.lm0 = (int)T.lm_row.size();
    sg.prow0 = T.nPr(); sg.lrow0 = T.nLr();
    sg.eo0 = EO.n(); sg.el0 = EL.n(); sg.ell0 = ELL.n(); sg.ep0 = EP.n();
    auto& vp = T.v2pose[g]; auto& vl = T.v2lm[g];
    vp.assign(G.nv(), -1); vl.assign(G.nv(), -1);
    for (int v = 0; v < G.nv(); ++v) {
      if (G.vtype[v] == VT_SE3) {
        vp[v] = (int)T.pose_row.size();
        T.pose_vertex.push_back(v);
        if (hidx[v] >= 0) { T.pose_row.push_back(T.nPr()); T.prow_pose.push_back(vp[v]); T.prow_graph.push_back(g); }
        else T.pose_row.push_back(-1);
      } else {
        vl[v] = (int)T.lm_row.size();
        T.lm_vertex.push_back(v);
        T.lm_kind.push_back((unsigned char)G.vtype[v]);
        T.has_planes |= G.vtype[v] == VT_PLANE;
        if (hidx[v] >= 0) { T.lm_row.push_back(T.nLr()); T.lrow_lm.push_back(vl[v]); T.lrow_graph.push_back(g); }
        else T.lm_row.push_back(-1);
      }
    }
    sg.npose = (int)T.pose_row.size() - sg.pose0; sg.nlm = (int)T.lm_row.size() - sg.lm0;
    sg.nprow = T.nPr() - sg.prow0; sg.nlrow = T.nLr() - sg.lrow0;
    for (int k = 0; k < G.ne(); ++k) {
      const EdgeType& et = kEdgeType[G.etype[k]];
      EdgeClassTab& C = T.cls[et.cls];
      C.a.push_back(et.vt_i == VT_SE3 ? vp[G.evi[k]] : vl[G.evi[k]]);
      C.b.push_back(et.vt_j < 0 ? -1 : (et.vt_j == VT_SE3 ? vp[G.evj[k]] : vl[G.evj[k]]));
      C.id.push_back(k); C.g.push_back(g); C.dim.push_back(et.d);
    }
    sg.neo = EO.n() - sg.eo0; sg.nel = EL.n() - sg.el0; sg.nell = ELL.n() - sg.ell0; sg.nep = EP.n() - sg.ep0;
    T.max_row_chunks = std::max(T.max_row_chunks, (sg.nprow * 6 + sg.nlrow * 3 + kRowChunk - 1) / kRowChunk);
    T.max_edge_chunks = std::max(T.max_edge_chunks, (sg.neo + sg.nel + sg.nell + sg.nep + kEdgeChunk - 1) / kEdgeChunk);
  }
  const int nPr = T.nPr(), nLr = T.nLr();
  // ---- SoA payloads: z and the upper triangle of Omega, zero-padded to the class's width
  for (int c = 0; c < kEdgeClasses; ++c) {
    EdgeClassTab& C = T.cls[c];
    const size_t n = (size_t)C.n();
    const int NZ = class_nz(c), D = class_d(c);
    C.z.resize((size_t)NZ * n); C.w.resize((size_t)upper_len(D) * n);
    for (size_t k = 0; k < n; ++k) {
      const HostGraph& G = *graphs[C.g[k]];
      const int s = C.id[k];
      const EdgeType& et = kEdgeType[G.etype[s]];
      for (int q = 0; q < NZ; ++q) C.z[(size_t)q * n + k] = q < et.nz ? G.meas[(size_t)s * 7 + q] : 0.0;
      pack_upper(&G.info[(size_t)s * 36], et.d, &C.w[k], D, n);
    }
  }
  // ---- unique off-diagonal blocks, owners and duplicates
  BlockIndex pp{T.ppoff, {}}, pl{T.plblk, {}}, ll{T.llblk, {}};
  // block of the edge whose ends are rows ra, rb (-1: not a row); ordered: the pair is stored (lower row, higher row)
  auto block_of = [](BlockIndex& ix, int ra, int rb, bool ordered) {
    if (ra < 0 || rb < 0 || (ordered && ra == rb)) return -1;
    return ordered ? ix.find_or_add(std::min(ra, rb), std::max(ra, rb)) : ix.find_or_add(ra, rb);
  };
  for (int k = 0; k < EO.n(); ++k) {
    const int ri = T.pose_row[EO.a[k]], rj = T.pose_row[EO.b[k]];
    const int idx = block_of(pp, ri, rj, true);
    EO.blk.push_back(idx < 0 ? -1 : idx * 2 + (ri > rj ? 1 : 0));
  }
  for (int k = 0; k < EL.n(); ++k) EL.blk.push_back(block_of(pl, T.pose_row[EL.a[k]], T.lm_row[EL.b[k]], false));
  for (int k = 0; k < ELL.n(); ++k) ELL.blk.push_back(block_of(ll, T.lm_row[ELL.a[k]], T.lm_row[ELL.b[k]], true));
  EP.blk.assign(EP.n(), -1);
  code_duplicates(EO.blk, 1, T.ppoff.size(), T.dup_eo);
  code_duplicates(EL.blk, 0, T.plblk.size(), T.dup_el);
  // ---- (row, incident edge) slots of the gather-form Jacobian build
  std::vector<std::vector<std::array<int, 4>>> pslots(nPr);
  std::vector<std::vector<int>> lslots(nLr), llblk_edges(T.llblk.size()), prior_rows(nPr);
  std::vector<std::vector<std::array<int, 2>>> llslots(nLr);
  std::vector<int> nse3(nPr, 0);
  for (int k = 0; k < EO.n(); ++k) {
    const int ri = T.pose_row[EO.a[k]], rj = T.pose_row[EO.b[k]];
    if (ri >= 0) { pslots[ri].push_back({k, 0, EO.a[k], EO.b[k]}); ++nse3[ri]; }
    if (rj >= 0) { pslots[rj].push_back({k, 1, EO.a[k], EO.b[k]}); ++nse3[rj]; }
  }
  for (int k = 0; k < EL.n(); ++k) {
    const int rp = T.pose_row[EL.a[k]], rl = T.lm_row[EL.b[k]];
    if (rp >= 0) pslots[rp].push_back({k, 2, EL.a[k], EL.b[k]});
    if (rl >= 0) lslots[rl].push_back(k);
  }
  for (int k = 0; k < ELL.n(); ++k) {
    const int ra = T.lm_row[ELL.a[k]], rb = T.lm_row[ELL.b[k]];
    if (ra >= 0) llslots[ra].push_back({k, 0});
    if (rb >= 0) llslots[rb].push_back({k, 1});
    if (ELL.blk[k] >= 0) llblk_edges[ELL.blk[k]].push_back(k);
  }
  for (int k = 0; k < EP.n(); ++k) { const int r = T.pose_row[EP.a[k]]; if (r >= 0) prior_rows[r].push_back(k); }
  auto same = [](const auto& x) { return x; };
  lists_to_csr(pslots, T.pslot_ptr, T.pslot_rec, same);
  lists_to_csr(lslots, T.lslot_ptr, T.lslot_edge, same);
  lists_to_csr(llslots, T.llslot_ptr, T.llslot_rec, same);
  lists_to_csr(llblk_edges, T.llblk_ptr, T.llblk_edge, same);
  lists_to_csr(prior_rows, T.ep_ptr, T.ep_edge, same, &T.ep_row);
  T.prow_perm.resize(nPr);
  for (int r = 0; r < nPr; ++r) T.prow_perm[r] = r;
  for (const GraphSeg& sg : T.seg)
    std::stable_sort(T.prow_perm.begin() + sg.prow0, T.prow_perm.begin() + sg.prow0 + sg.nprow, [&](int x, int y) {
      if (nse3[x] != nse3[y]) return nse3[x] < nse3[y];
      return pslots[x].size() < pslots[y].size();
    });
  // ---- layout of H
  const int nPP = (int)T.ppoff.size(), nPL = (int)T.plblk.size(), nLL = (int)T.llblk.size();
  T.hll_base = (int64_t)nPr * 36;
  T.hpp_off_base = T.hll_base + (((int64_t)nLr * 9 + 1) & ~(int64_t)1);   // even: the 6-wide blocks behind it stay 16-byte aligned
  T.hpl_base = T.hpp_off_base + (int64_t)nPP * 36;
  T.hll_off_base = T.hpl_base + (int64_t)nPL * 18;
  T.h_total = T.hll_off_base + (int64_t)nLL * 9;
  if (T.h_total >= (int64_t)1 << 31) return T;   // block offsets are int32: the caller refuses the batch
  // ---- adjacency: {offset of the block in H, offset of the column in x, format}
  std::vector<std::vector<std::array<int, 3>>> adj(nPr + nLr);
  for (int i = 0; i < nPP; ++i) {
    const int a = T.ppoff[i].first, c = T.ppoff[i].second, off = (int)(T.hpp_off_base + (int64_t)i * 36);
    adj[a].push_back({off, 6 * c, 0});
    adj[c].push_back({off, 6 * a, 1});
  }
  for (int i = 0; i < nPL; ++i) {
    const int rp = T.plblk[i].first, rl = T.plblk[i].second, off = (int)(T.hpl_base + (int64_t)i * 18);
    adj[rp].push_back({off, 6 * nPr + 3 * rl, 2});
    adj[nPr + rl].push_back({off, 6 * rp, 3});
  }
  for (int i = 0; i < nLL; ++i) {
    const int a = T.llblk[i].first, c = T.llblk[i].second, off = (int)(T.hll_off_base + (int64_t)i * 9);
    adj[nPr + a].push_back({off, 6 * nPr + 3 * c, 4});
    adj[nPr + c].push_back({off, 6 * nPr + 3 * a, 5});
  }
  for (auto& row : adj) std::sort(row.begin(), row.end(), [](const std::array<int, 3>& x, const std::array<int, 3>& y) { return x[1] < y[1]; });
  std::vector<int> unused;
  lists_to_csr(adj, T.adj_ptr, T.adj_blk, [](const std::array<int, 3>& x) { return x[0]; });
  lists_to_csr(adj, unused, T.adj_x, [](const std::array<int, 3>& x) { return x[1]; });
  lists_to_csr(adj, unused, T.adj_fmt, [](const std::array<int, 3>& x) { return (unsigned char)x[2]; });
  return T;
}

}  // namespace sslam
