// Host-side entry points of libgcrnn_hip.so: version/status strings and graph preparation
// (dense GSO -> CSR, degree ordering). No GPU is touched here, so these run in CPU-only tests.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>
#include "../../include/gcrnn.h"
#include "gcrnn_readout.h"
#include "gcrnn_rnn.h"

extern "C" int gcrnn_version(void) { return 121; }  // 0.1.21 (round 5: hand-allocated-hop forward kernel, node-gated passes on the wide kernel, chunk pairs in the weight-gradient kernel)

extern "C" const char* gcrnn_status_string(int status) {
  switch (status) {
    case GCRNN_OK: return "ok";
    case GCRNN_ERR_BAD_DTYPE: return "unsupported dtype for this entry point";
    case GCRNN_ERR_BAD_SHAPE: return "bad shape (zero/negative size or a grid limit exceeded)";
    case GCRNN_ERR_NULL_POINTER: return "null pointer for a required argument";
    case GCRNN_ERR_UNSUPPORTED: return "unsupported argument combination";
    case GCRNN_ERR_LAUNCH: return "HIP kernel launch failed";
    case GCRNN_ERR_WORKSPACE: return "workspace too small";
    default: return "unknown status";
  }
}

// last HIP runtime error seen by a launch check (diagnostics for GCRNN_ERR_LAUNCH)
static thread_local char g_last_hip_error[256] = "";
extern "C" void gcrnn_note_hip_error(int code, const char* what) {
  snprintf(g_last_hip_error, sizeof(g_last_hip_error), "hip error %d: %s", code, what ? what : "?");
}
extern "C" const char* gcrnn_last_hip_error(void) { return g_last_hip_error; }

static inline bool keep(double v, double tol) { return std::fabs(v) > tol; }

// entry (i, j) of the operator whose CSR we build: S^T[i][j] = S[j][i]; identity optionally added
static inline double entry(const double* S, int64_t N, int transpose, int add_identity, int64_t i, int64_t j) {
  double v = transpose ? S[j * N + i] : S[i * N + j];
  if (add_identity && i == j) v += 1.0;
  return v;
}

extern "C" int gcrnn_csr_count(const double* S, int64_t N, int transpose, int add_identity, double tol, int64_t* nnz) {
  if (!S || !nnz) return GCRNN_ERR_NULL_POINTER;
  if (N <= 0 || tol < 0) return GCRNN_ERR_BAD_SHAPE;
  int64_t c = 0;
  for (int64_t i = 0; i < N; ++i)
    for (int64_t j = 0; j < N; ++j) c += keep(entry(S, N, transpose, add_identity, i, j), tol);
  *nnz = c;
  return GCRNN_OK;
}

extern "C" int gcrnn_csr_fill(const double* S, int64_t N, int transpose, int add_identity, double tol, int32_t* rowptr,
                              int32_t* col, double* val) {
  if (!S || !rowptr) return GCRNN_ERR_NULL_POINTER;
  if (N <= 0 || N > 2147483647LL || tol < 0) return GCRNN_ERR_BAD_SHAPE;
  int64_t c = 0;
  rowptr[0] = 0;
  for (int64_t i = 0; i < N; ++i) {
    for (int64_t j = 0; j < N; ++j) {
      const double v = entry(S, N, transpose, add_identity, i, j);
      if (keep(v, tol)) {
        if (c >= 2147483647LL) return GCRNN_ERR_BAD_SHAPE;
        if (col) col[c] = (int32_t)j;
        if (val) val[c] = v;
        ++c;
      }
    }
    rowptr[i + 1] = (int32_t)c;
  }
  return GCRNN_OK;
}

extern "C" int gcrnn_degree_order(const int32_t* rowptr, int64_t N, int32_t* order) {
  if (!rowptr || !order) return GCRNN_ERR_NULL_POINTER;
  if (N <= 0 || N > 2147483647LL) return GCRNN_ERR_BAD_SHAPE;
  std::iota(order, order + N, 0);
  std::stable_sort(order, order + N, [rowptr](int32_t a, int32_t b) {
    return (rowptr[a + 1] - rowptr[a]) > (rowptr[b + 1] - rowptr[b]);
  });
  return GCRNN_OK;
}

// ---- sliced ELL for the fused kernels ---------------------------------------------------------
// Slot p of the tiling works on node order[p]; tiles of `tile` slots. Tile t stores
// deg_t = max degree in the tile rounded up to `pad` entries per slot, laid out [entry][slot-in-tile] so that
// one wave reads 16 consecutive (col, val) pairs per entry. col = neighbour node id (natural numbering);
// padding entries are (0, 0.0).
static int ell_tile_deg(const int32_t* rowptr, const int32_t* order, int64_t N, int64_t t, int tile, int pad) {
  int d = 0;
  for (int r = 0; r < tile; ++r) {
    const int64_t p = t * tile + r;
    if (p < N) {
      const int32_t n = order ? order[p] : (int32_t)p;
      d = std::max(d, rowptr[n + 1] - rowptr[n]);
    }
  }
  return (d + pad - 1) / pad * pad;
}

extern "C" int gcrnn_ell_size(const int32_t* rowptr, int64_t N, const int32_t* order, int tile, int pad,
                              int64_t ntiles, int64_t* nentries) {
  if (!rowptr || !nentries) return GCRNN_ERR_NULL_POINTER;
  if (N <= 0 || tile <= 0 || pad <= 0 || ntiles * tile < N) return GCRNN_ERR_BAD_SHAPE;
  int64_t tot = 0;
  for (int64_t t = 0; t < ntiles; ++t) tot += ell_tile_deg(rowptr, order, N, t, tile, pad);
  *nentries = tot;   // in units of `tile` (col,val) pairs
  return GCRNN_OK;
}

// ---- bank-conflict-aware entry scheduling -------------------------------------------------------------------
// The fused kernel keeps the hop state in LDS as 64-byte rows (16 fp32 per node) whose four 16-byte quads are
// XOR-swizzled by the node id: quad q of node n sits in slot q ^ ((n >> 2) & 3). A ds_read_b128 is served in
// four groups of 16 lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...: MI355X_MICROARCH.md, LDS table); lane
// (r = l & 15, q = l >> 4) reads quad q of the e-th neighbour of the tile's slot r. With the swizzle, all four
// groups are conflict-free exactly when the 16 keys
//     key_r = (col_r & 15)        for r in {0-3, 12-15}
//     key_r = (col_r & 15) ^ 4    for r in {4-11}
// are distinct. The order of a row's neighbours is free and padding entries (weight 0) may point at any row, so
// for every entry index we pick, per slot, an unused neighbour by maximum bipartite matching (slots x keys).
//
// Generalisation: the LDS row of a node and the XOR swizzle of its quads are free per node. node_addr[n] =
// (row << 6) | (swz << 4) is the byte-offset code of node n's state row (NULL = the identity layout above: row n,
// swz = (n >> 2) & 3). The bank-quad of node n seen by a lane with quad q is ((row & 3) << 2 | swz ^ q), so the node's
// 4-bit key is key4 = (swz << 2) | (row & 3), and slots 4..11 see key4 ^ 4. gcrnn_ell_assign_rows picks the keys that
// flatten every tile's key histogram (local search); rows are then dealt out within each (row & 3) class.
static inline int node_key4(const int32_t* node_addr, int32_t col) {
  if (!node_addr) return col & 15;
  const int32_t a = node_addr[col];
  return (((a >> 4) & 3) << 2) | ((a >> 6) & 3);
}
static inline int ell_key(int r, int32_t col, const int32_t* node_addr) {
  const int k = node_key4(node_addr, col);
  return (r >= 4 && r < 12) ? (k ^ 4) : k;
}

namespace {
struct TileSched {
  // per slot: remaining neighbours (col, val)
  std::vector<std::pair<int32_t, float>> rem[16];
  int pads[16];
  int match_key[16];   // key -> slot
  const int32_t* node_addr = nullptr;
  bool try_slot(int r, bool used_key[16], int key_of[16], int depth) {
    // candidate keys of slot r: keys of its unused neighbours (wildcards are handled by the caller)
    for (size_t i = 0; i < rem[r].size(); ++i) {
      const int k = ell_key(r, rem[r][i].first, node_addr);
      if (used_key[k]) continue;
      used_key[k] = true;
      if (match_key[k] < 0 || try_slot(match_key[k], used_key, key_of, depth + 1)) {
        match_key[k] = r;
        key_of[r] = k;
        return true;
      }
    }
    return false;
  }
};

// Exact schedule of one tile whose key histogram fits (every key at most d times): pad the slots x keys multigraph with
// zero-weight wildcard edges to a d-regular bipartite multigraph and peel off d perfect matchings (Koenig) -- every entry
// is conflict-free. M[r][k] = real edges, Dm[r][k] = wildcard edges.
struct RegularPeel {
  int M[16][16], Dm[16][16];
  int mk[16];            // key -> slot of the current matching
  bool aug(int r, bool seen[16]) {
    for (int k = 0; k < 16; ++k) {
      if (M[r][k] + Dm[r][k] == 0 || seen[k]) continue;
      seen[k] = true;
      if (mk[k] < 0 || aug(mk[k], seen)) { mk[k] = r; return true; }
    }
    return false;
  }
  bool perfect(int key_of[16]) {
    for (int k = 0; k < 16; ++k) mk[k] = -1;
    for (int r = 0; r < 16; ++r) {
      bool seen[16] = {false};
      if (!aug(r, seen)) return false;
    }
    for (int k = 0; k < 16; ++k) key_of[mk[k]] = k;
    return true;
  }
};
}  // namespace

extern "C" int gcrnn_ell_fill(const int32_t* rowptr, const int32_t* col, const double* val, int64_t N,
                              const int32_t* order, int tile, int pad, int64_t ntiles, const int32_t* node_addr,
                              int32_t* tile_off, int32_t* ell_col, float* ell_val) {
  return gcrnn_ell_fill_z(rowptr, col, val, N, order, tile, pad, ntiles, node_addr, -1, tile_off, ell_col, ell_val);
}

// zero_from >= 0: the nodes zero_from .. N-1 are padding rows whose state is always zero; every zero-weight padding entry then
// points at one of THEM (with the bank key the schedule wants), so that a kernel may drop the weights of a uniform-weight graph
// and sum the gathered rows directly. GCRNN_ERR_UNSUPPORTED when the padding rows do not cover all 16 bank keys.
extern "C" int gcrnn_ell_fill_z(const int32_t* rowptr, const int32_t* col, const double* val, int64_t N,
                                const int32_t* order, int tile, int pad, int64_t ntiles, const int32_t* node_addr,
                                int64_t zero_from, int32_t* tile_off, int32_t* ell_col, float* ell_val) {
  if (!rowptr || !col || !val || !tile_off || !ell_col || !ell_val) return GCRNN_ERR_NULL_POINTER;
  if (N <= 0 || tile <= 0 || pad <= 0 || ntiles * tile < N) return GCRNN_ERR_BAD_SHAPE;
  const bool schedule = (tile == 16);
  int64_t off = 0;
  TileSched ts;
  ts.node_addr = node_addr;
  // a node for every key: where zero-weight padding entries point (rows 0..15 carry all 16 keys in the identity layout)
  int32_t node_of_key[16];
  for (int k = 0; k < 16; ++k) node_of_key[k] = -1;
  if (schedule)
    for (int64_t n = (zero_from >= 0 ? zero_from : 0); n < N; ++n) {
      const int k = node_key4(node_addr, (int32_t)n);
      if (node_of_key[k] < 0) node_of_key[k] = (int32_t)n;
    }
  if (zero_from >= 0) {
    if (!schedule || zero_from > N) return GCRNN_ERR_BAD_SHAPE;
    for (int k = 0; k < 16; ++k) if (node_of_key[k] < 0) return GCRNN_ERR_UNSUPPORTED;
  }
  for (int k = 0; k < 16; ++k) if (node_of_key[k] < 0) node_of_key[k] = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    tile_off[t] = (int32_t)off;
    const int d = ell_tile_deg(rowptr, order, N, t, tile, pad);
    if (!schedule) {
      for (int e = 0; e < d; ++e)
        for (int r = 0; r < tile; ++r) {
          const int64_t p = t * tile + r;
          int32_t c = 0;
          float v = 0.f;
          if (p < N) {
            const int32_t n = order ? order[p] : (int32_t)p;
            const int32_t j = rowptr[n] + e;
            if (j < rowptr[n + 1]) { c = col[j]; v = (float)val[j]; }
          }
          ell_col[(off + e) * tile + r] = c;
          ell_val[(off + e) * tile + r] = v;
        }
    } else {
      for (int r = 0; r < 16; ++r) {
        ts.rem[r].clear();
        const int64_t p = t * 16 + r;
        if (p < N) {
          const int32_t n = order ? order[p] : (int32_t)p;
          for (int32_t j = rowptr[n]; j < rowptr[n + 1]; ++j) ts.rem[r].push_back({col[j], (float)val[j]});
        }
        ts.pads[r] = d - (int)ts.rem[r].size();
      }
      // exact conflict-free schedule when no key is wanted more than d times
      {
        RegularPeel rp;
        int kdeg[16] = {0};
        for (int r = 0; r < 16; ++r)
          for (int k = 0; k < 16; ++k) rp.M[r][k] = rp.Dm[r][k] = 0;
        for (int r = 0; r < 16; ++r)
          for (auto& cv : ts.rem[r]) { const int k = ell_key(r, cv.first, node_addr); ++rp.M[r][k]; ++kdeg[k]; }
        int kmax = 0;
        for (int k = 0; k < 16; ++k) kmax = std::max(kmax, kdeg[k]);
        if (d > 0 && kmax <= d) {
          int rdef[16], kdef[16];
          for (int r = 0; r < 16; ++r) rdef[r] = ts.pads[r];
          for (int k = 0; k < 16; ++k) kdef[k] = d - kdeg[k];
          for (int r = 0; r < 16; ++r)
            for (int k = 0; k < 16 && rdef[r] > 0; ++k) {
              const int x = std::min(rdef[r], kdef[k]);
              rp.Dm[r][k] += x; rdef[r] -= x; kdef[k] -= x;
            }
          bool ok = true;
          for (int e = 0; e < d && ok; ++e) {
            int key_of[16];
            ok = rp.perfect(key_of);
            if (!ok) break;
            for (int r = 0; r < 16; ++r) {
              const int k = key_of[r];
              int32_t c; float v;
              if (rp.M[r][k] > 0) {
                --rp.M[r][k];
                size_t i = 0;
                while (ell_key(r, ts.rem[r][i].first, node_addr) != k) ++i;
                c = ts.rem[r][i].first; v = ts.rem[r][i].second;
                ts.rem[r].erase(ts.rem[r].begin() + i);
              } else {
                --rp.Dm[r][k];
                c = node_of_key[(r >= 4 && r < 12) ? (k ^ 4) : k]; v = 0.f;
              }
              ell_col[(off + e) * 16 + r] = c;
              ell_val[(off + e) * 16 + r] = v;
            }
          }
          if (ok) { off += d; if (off > 2147483647LL / tile) return GCRNN_ERR_BAD_SHAPE; continue; }
          // (cannot happen for a regular multigraph; fall through to the greedy schedule on a fresh copy)
          for (int r = 0; r < 16; ++r) {
            ts.rem[r].clear();
            const int64_t p = t * 16 + r;
            if (p < N) {
              const int32_t n = order ? order[p] : (int32_t)p;
              for (int32_t j = rowptr[n]; j < rowptr[n + 1]; ++j) ts.rem[r].push_back({col[j], (float)val[j]});
            }
            ts.pads[r] = d - (int)ts.rem[r].size();
          }
        }
      }
      for (int e = 0; e < d; ++e) {
        int key_of[16];
        for (int r = 0; r < 16; ++r) key_of[r] = -1;
        for (int k = 0; k < 16; ++k) ts.match_key[k] = -1;
        // slots that MUST take a real neighbour now (no padding left) first, then the rest, fewest options first
        int ord[16];
        for (int r = 0; r < 16; ++r) ord[r] = r;
        std::stable_sort(ord, ord + 16, [&](int a, int b) {
          const bool fa = ts.pads[a] == 0, fb = ts.pads[b] == 0;
          if (fa != fb) return fa;
          return ts.rem[a].size() < ts.rem[b].size();
        });
        for (int oi = 0; oi < 16; ++oi) {
          const int r = ord[oi];
          if (ts.rem[r].empty()) continue;
          bool used[16] = {false};
          ts.try_slot(r, used, key_of, 0);
        }
        // keys still free go to padding wildcards; unmatched slots without padding take any neighbour (a conflict)
        bool key_taken[16];
        for (int k = 0; k < 16; ++k) key_taken[k] = ts.match_key[k] >= 0;
        for (int r = 0; r < 16; ++r) {
          int32_t c = 0;
          float v = 0.f;
          if (key_of[r] >= 0) {
            for (size_t i = 0; i < ts.rem[r].size(); ++i)
              if (ell_key(r, ts.rem[r][i].first, node_addr) == key_of[r]) {
                c = ts.rem[r][i].first; v = ts.rem[r][i].second;
                ts.rem[r].erase(ts.rem[r].begin() + i);
                break;
              }
          } else if (ts.pads[r] > 0) {
            int k = 0;
            while (k < 16 && key_taken[k]) ++k;
            if (k == 16) k = 0;
            key_taken[k] = true;
            c = node_of_key[(r >= 4 && r < 12) ? (k ^ 4) : k];      // any node with that key
            v = 0.f;
            --ts.pads[r];
          } else {
            c = ts.rem[r].back().first; v = ts.rem[r].back().second;
            ts.rem[r].pop_back();
          }
          ell_col[(off + e) * 16 + r] = c;
          ell_val[(off + e) * 16 + r] = v;
        }
      }
    }
    off += d;
    if (off > 2147483647LL / tile) return GCRNN_ERR_BAD_SHAPE;
  }
  tile_off[ntiles] = (int32_t)off;
  return GCRNN_OK;
}

// LDS cycles the four 16-lane groups of one gather need, summed over all entries, under the swizzled layout
// (diagnostic: 4 * entries = conflict-free).
extern "C" int gcrnn_ell_conflict_cycles(const int32_t* ell_col, int64_t entries, const int32_t* node_addr, int64_t* cycles) {
  if (!ell_col || !cycles) return GCRNN_ERR_NULL_POINTER;
  int64_t tot = 0;
  for (int64_t e = 0; e < entries; ++e) {
    int cnt[16] = {0};
    int mx = 0;
    for (int r = 0; r < 16; ++r) mx = std::max(mx, ++cnt[ell_key(r, ell_col[e * 16 + r], node_addr)]);
    tot += 4 * mx;
  }
  *cycles = tot;
  return GCRNN_OK;
}

// Pack a 16-slot ELL into the LDS image of the fused kernel: groups of 4 entries,
//   val4[g][r][4] fp32 weights;  col4[g][r][4] u16 = node_addr[col] = (row << 6) | (swz << 4)   (row offset | swizzle bits)
extern "C" int gcrnn_ell_pack_lds(const int32_t* ell_col, const float* ell_val, int64_t entries, const int32_t* node_addr,
                                  float* val4, uint16_t* col4) {
  if (!ell_col || !ell_val || !val4 || !col4) return GCRNN_ERR_NULL_POINTER;
  if (entries < 0 || entries % 4) return GCRNN_ERR_BAD_SHAPE;
  for (int64_t g = 0; g < entries / 4; ++g)
    for (int r = 0; r < 16; ++r)
      for (int p = 0; p < 4; ++p) {
        const int32_t c = ell_col[(g * 4 + p) * 16 + r];
        if (c < 0 || c >= 1024) return GCRNN_ERR_BAD_SHAPE;
        val4[(g * 16 + r) * 4 + p] = ell_val[(g * 4 + p) * 16 + r];
        col4[(g * 16 + r) * 4 + p] = (uint16_t)(node_addr ? node_addr[c] : ((c << 6) | (((c >> 2) & 3) << 4)));
      }
  return GCRNN_OK;
}

// Choose the LDS row and quad swizzle of every node (see the key model above) so that, for every tile, no key is wanted
// by more neighbours than the tile has entries -- then gcrnn_ell_fill's exact schedule leaves no bank conflict at all.
// Local search: nodes are visited in a fixed pseudo-random order; each takes the key that minimises
// (sum over its tiles of max(d_t, busiest key), sum of squared overloads). Rows: class (row & 3) holds at most N / 4 nodes.
// N = padded node count (multiple of 16, at most 1024), rowptr / order as for gcrnn_ell_fill (tile = 16).
extern "C" int gcrnn_ell_assign_rows(const int32_t* rowptr, const int32_t* col, int64_t N, const int32_t* order, int pad,
                                     int64_t ntiles, int32_t* node_addr) {
  return gcrnn_ell_assign_rows_z(rowptr, col, N, order, pad, ntiles, -1, node_addr);
}

// Write-aware key search (default). A node's 4-bit gather key is key4 = swz << 2 | (row & 3); the state write-backs
// (ds_write_b128: 8 groups of 8 contiguous lanes on 32 banks = 8 bank quads; lane = slot + 16 quad, address = row << 6 | (swz ^ quad) << 4)
// are conflict-free exactly when the 8 slots of every HALF TILE sit on 8 different write keys wkey = (row & 1) << 2 | swz. That is kept
// as a hard constraint: each half tile holds a permutation of the 8 write keys; bit 1 of the row class is free. The search moves inside
// that space -- exchange the keys of two slots of one half tile; exchange the free bit of two nodes of equal row parity (the four row
// classes stay at N / 4 nodes each) -- and minimises the gather cycles of the tiles (sum over tiles of max(depth, largest key count)),
// then the squared overshoot. A pure function of the graph (fixed pseudo-random visiting order).
namespace {
struct KeySearch {
  int64_t N, ntiles;
  std::vector<std::vector<std::pair<int, int>>> in;     // node -> (tile, flip) of every slot that gathers it
  std::vector<int> depth, key;
  std::vector<std::array<int, 16>> cnt;
  std::vector<int> touched;
  std::vector<int> stamp;
  int epoch = 0;
  void add(int32_t n, int d) { for (auto& e : in[n]) cnt[e.first][key[n] ^ e.second] += d; }
  void mark(int32_t n) {
    for (auto& e : in[n]) if (stamp[e.first] != epoch) { stamp[e.first] = epoch; touched.push_back(e.first); }
  }
  void cost(long& c1, long& c2) const {
    c1 = 0; c2 = 0;
    for (int t : touched) {
      int mx = 0;
      for (int q = 0; q < 16; ++q) {
        mx = std::max(mx, cnt[t][q]);
        const int over = cnt[t][q] - depth[t] + 1;
        if (over > 0) c2 += (long)over * over;
      }
      c1 += std::max(depth[t], mx);
    }
  }
  // exchange-type move on two nodes: keys become (ka, kb); returns true (and keeps it) when the cost drops
  bool try_move(int32_t a, int32_t b, int ka, int kb) {
    ++epoch; touched.clear(); mark(a); mark(b);
    if (touched.empty()) return false;
    long p1, p2, q1, q2;
    cost(p1, p2);
    const int oa = key[a], ob = key[b];
    add(a, -1); add(b, -1); key[a] = ka; key[b] = kb; add(a, 1); add(b, 1);
    cost(q1, q2);
    if (q1 < p1 || (q1 == p1 && q2 < p2)) return true;
    add(a, -1); add(b, -1); key[a] = oa; key[b] = ob; add(a, 1); add(b, 1);
    return false;
  }
};
}  // namespace

static int assign_rows_write_aware(const int32_t* rowptr, const int32_t* col, int64_t N, const int32_t* order, int pad,
                                   int64_t ntiles, int64_t zero_from, int32_t* node_addr) {
  KeySearch ks;
  ks.N = N; ks.ntiles = ntiles;
  ks.depth.resize(ntiles);
  for (int64_t t = 0; t < ntiles; ++t) ks.depth[t] = ell_tile_deg(rowptr, order, N, t, 16, pad);
  ks.in.assign(N, {});
  std::vector<int> half(N, -1);
  for (int64_t p = 0; p < N; ++p) {
    const int32_t n = order ? order[p] : (int32_t)p;
    if (n < 0 || n >= N || half[n] >= 0) return GCRNN_ERR_BAD_SHAPE;        // every node sits in exactly one slot
    half[n] = (int)(p >> 3);
    const int t = (int)(p >> 4), r = (int)(p & 15);
    for (int32_t j = rowptr[n]; j < rowptr[n + 1]; ++j) {
      if (col[j] < 0 || col[j] >= N) return GCRNN_ERR_BAD_SHAPE;
      ks.in[col[j]].push_back({t, (r >= 4 && r < 12) ? 4 : 0});
    }
  }
  const int64_t nhalf = N / 8;
  std::vector<std::array<int32_t, 8>> member(nhalf);
  std::vector<int> fill(nhalf, 0);
  for (int64_t p = 0; p < N; ++p) member[p >> 3][fill[p >> 3]++] = order ? order[p] : (int32_t)p;
  auto key_of = [](int w, int b1) { return ((w & 3) << 2) | (b1 << 1) | (w >> 2); };
  ks.key.assign(N, -1);
  std::vector<char> fixed(N, 0);
  int cls[4] = {0, 0, 0, 0};
  if (zero_from >= 0)
    for (int64_t n = zero_from; n < N && n - zero_from < 16; ++n) {
      if (rowptr[n + 1] != rowptr[n] || !ks.in[n].empty()) return GCRNN_ERR_BAD_SHAPE;   // a padding row has no edges
      const int i = (int)(n - zero_from);                     // one zero row per gather key; any 8 consecutive ones differ in the write key
      ks.key[n] = key_of(i & 7, i >> 3);
      fixed[n] = 1;
      ++cls[ks.key[n] & 3];
    }
  for (int64_t h = 0; h < nhalf; ++h) {
    bool used[8] = {false};
    for (int32_t n : member[h]) if (fixed[n]) {
      const int w = ((ks.key[n] & 1) << 2) | (ks.key[n] >> 2);
      if (used[w]) return GCRNN_ERR_UNSUPPORTED;
      used[w] = true;
    }
    int w = 0;
    for (int32_t n : member[h]) {
      if (fixed[n]) continue;
      while (used[w]) ++w;
      used[w] = true;
      const int b0 = w >> 2;
      const int b1 = cls[2 | b0] < cls[b0] ? 1 : 0;           // keep the two classes of this row parity level
      ks.key[n] = key_of(w, b1);
      ++cls[ks.key[n] & 3];
    }
  }
  if (cls[0] != N / 4 || cls[1] != N / 4 || cls[2] != N / 4 || cls[3] != N / 4) return GCRNN_ERR_UNSUPPORTED;
  ks.cnt.assign(ntiles, {});
  for (auto& c : ks.cnt) c.fill(0);
  ks.stamp.assign(ntiles, 0);
  for (int64_t n = 0; n < N; ++n) ks.add((int32_t)n, 1);
  std::vector<int32_t> visit(N);
  std::iota(visit.begin(), visit.end(), 0);
  uint64_t lcg = 0x9E3779B97F4A7C15ull;
  auto rnd = [&](uint64_t m) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (lcg >> 33) % m; };
  for (int64_t i = N - 1; i > 0; --i) std::swap(visit[i], visit[rnd((uint64_t)(i + 1))]);
  for (int pass = 0; pass < 12; ++pass) {
    bool changed = false;
    for (int64_t vi = 0; vi < N; ++vi) {
      const int32_t a = visit[vi];
      if (fixed[a]) continue;
      // (1) exchange keys with another slot of the same half tile
      for (int32_t b : member[half[a]]) {
        if (b == a || fixed[b] || ks.key[a] == ks.key[b]) continue;
        if (ks.in[a].empty() && ks.in[b].empty()) continue;
        if (ks.try_move(a, b, ks.key[b], ks.key[a])) changed = true;
      }
      // (2) exchange the free row bit with a node of the same row parity (a few pseudo-random partners)
      if (!ks.in[a].empty())
        for (int tries = 0; tries < 12; ++tries) {
          const int32_t b = (int32_t)rnd((uint64_t)N);
          if (b == a || fixed[b]) continue;
          if (((ks.key[a] ^ ks.key[b]) & 3) != 2) continue;   // same parity, other free bit
          if (ks.try_move(a, b, ks.key[a] ^ 2, ks.key[b] ^ 2)) changed = true;
        }
    }
    if (!changed) break;
  }
  int next_row[4] = {0, 1, 2, 3};
  for (int64_t n = 0; n < N; ++n) {
    const int a = ks.key[n] & 3;
    if (next_row[a] >= N) return GCRNN_ERR_WORKSPACE;
    node_addr[n] = (next_row[a] << 6) | ((ks.key[n] >> 2) << 4);
    next_row[a] += 4;
  }
  return GCRNN_OK;
}

// zero_from >= 0: the first 16 padding rows zero_from .. zero_from+15 get the bank keys 0 .. 15 (fixed, not searched), so that
// gcrnn_ell_fill_z finds a zero row for every key.
extern "C" int gcrnn_ell_assign_rows_z(const int32_t* rowptr, const int32_t* col, int64_t N, const int32_t* order, int pad,
                                       int64_t ntiles, int64_t zero_from, int32_t* node_addr) {
  if (!rowptr || !col || !node_addr) return GCRNN_ERR_NULL_POINTER;
  if (N <= 0 || N > 1024 || N % 16 || pad <= 0 || ntiles * 16 < N) return GCRNN_ERR_BAD_SHAPE;
  if (!getenv("GCRNN_PLAN_LEGACY_KEYS")) {                      // A/B switch: the round-1 search below looks at the gathers only
    const int rc = assign_rows_write_aware(rowptr, col, N, order, pad, ntiles, zero_from, node_addr);
    if (rc != GCRNN_ERR_UNSUPPORTED) return rc;
  }
  std::vector<int> depth(ntiles);
  for (int64_t t = 0; t < ntiles; ++t) depth[t] = ell_tile_deg(rowptr, order, N, t, 16, pad);
  // incoming edges of every node: (tile, flip) with flip = 4 for slots 4..11
  std::vector<std::vector<std::pair<int, int>>> in(N);
  for (int64_t t = 0; t < ntiles; ++t)
    for (int r = 0; r < 16; ++r) {
      const int64_t p = t * 16 + r;
      if (p >= N) continue;
      const int32_t n = order ? order[p] : (int32_t)p;
      for (int32_t j = rowptr[n]; j < rowptr[n + 1]; ++j) {
        if (col[j] < 0 || col[j] >= N) return GCRNN_ERR_BAD_SHAPE;
        in[col[j]].push_back({(int)t, (r >= 4 && r < 12) ? 4 : 0});
      }
    }
  std::vector<int> key(N);
  std::vector<std::array<int, 16>> cnt(ntiles);
  for (auto& c : cnt) c.fill(0);
  int cls[4] = {0, 0, 0, 0};
  std::vector<char> fixed(N, 0);
  for (int64_t n = 0; n < N; ++n) {
    key[n] = (int)(n & 15);
    if (zero_from >= 0 && n >= zero_from) {
      if (!in[n].empty()) return GCRNN_ERR_BAD_SHAPE;         // a padding row has no edges
      if (n - zero_from < 16) {                               // one zero row per key; further padding rows stay free (slack for the search)
        key[n] = (int)(n - zero_from);
        fixed[n] = 1;
        ++cls[key[n] & 3];
      }
    }
    if (!in[n].empty()) ++cls[n & 3];                         // nodes nobody gathers (padding rows, sinks) take leftover rows
    for (auto& e : in[n]) ++cnt[e.first][key[n] ^ e.second];
  }
  const int cap = (int)(N / 4);
  std::vector<int32_t> visit(N);
  std::iota(visit.begin(), visit.end(), 0);
  uint64_t lcg = 0x9E3779B97F4A7C15ull;
  for (int64_t i = N - 1; i > 0; --i) {                      // fixed shuffle: the plan is a pure function of the graph
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    std::swap(visit[i], visit[(lcg >> 33) % (uint64_t)(i + 1)]);
  }
  std::vector<int> tiles;
  for (int pass = 0; pass < 8; ++pass) {
    bool changed = false;
    for (int64_t vi = 0; vi < N; ++vi) {
      const int32_t n = visit[vi];
      if (in[n].empty()) continue;
      tiles.clear();
      for (auto& e : in[n]) tiles.push_back(e.first);
      std::sort(tiles.begin(), tiles.end());
      tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
      const int k0 = key[n];
      for (auto& e : in[n]) --cnt[e.first][k0 ^ e.second];
      long best1 = -1, best2 = -1;
      int bestk = k0;
      for (int kk = 0; kk < 16; ++kk) {
        const int k = (k0 + kk) & 15;                          // the current key first: ties keep it
        if ((k & 3) != (k0 & 3) && cls[k & 3] >= cap) continue;
        for (auto& e : in[n]) ++cnt[e.first][k ^ e.second];
        long c1 = 0, c2 = 0;
        for (int t : tiles) {
          int mx = 0;
          for (int q = 0; q < 16; ++q) {
            mx = std::max(mx, cnt[t][q]);
            const int over = cnt[t][q] - depth[t] + 1;
            if (over > 0) c2 += (long)over * over;
          }
          c1 += std::max(depth[t], mx);
        }
        for (auto& e : in[n]) --cnt[e.first][k ^ e.second];
        if (best1 < 0 || c1 < best1 || (c1 == best1 && c2 < best2)) { best1 = c1; best2 = c2; bestk = k; }
      }
      if (bestk != k0) { changed = true; --cls[k0 & 3]; ++cls[bestk & 3]; key[n] = bestk; }
      for (auto& e : in[n]) ++cnt[e.first][bestk ^ e.second];
    }
    if (!changed) break;
  }
  int next_row[4] = {0, 1, 2, 3};
  for (int64_t n = 0; n < N; ++n) {
    if (in[n].empty() && !fixed[n]) continue;
    const int a = key[n] & 3;
    const int row = next_row[a];
    next_row[a] += 4;
    if (row >= N) return GCRNN_ERR_WORKSPACE;                  // cannot happen: class sizes are capped at N / 4
    node_addr[n] = (row << 6) | ((key[n] >> 2) << 4);
  }
  int a = 0;
  for (int64_t n = 0; n < N; ++n) {
    if (!in[n].empty() || fixed[n]) continue;
    while (a < 4 && next_row[a] >= N) ++a;
    if (a == 4) return GCRNN_ERR_WORKSPACE;
    node_addr[n] = (next_row[a] << 6) | ((key[n] >> 2) << 4);
    next_row[a] += 4;
  }
  return GCRNN_OK;
}

// ---- graph-filter layer (gcrnn_readout.hip): envelope and slot count, host logic only ---------------------------------------
static int64_t gfl_lds(int dtype, int64_t N, int64_t nnz, int64_t F_in, int64_t F_out, int64_t K, int uniform) {
  const int64_t acc = dtype == GCRNN_F64 ? 8 : 4;
  const int64_t f = gfl_layout(N, nnz, F_in, F_out, K, acc, 0, uniform).total, b = gfl_layout(N, nnz, F_in, F_out, K, acc, 1, uniform).total;
  return f > b ? f : b;
}

extern "C" int gcrnn_graph_filter_layer_supported(int dtype, int64_t N, int64_t nnz, int64_t E, int64_t F_in, int64_t F_out, int64_t K,
                                                  int uniform) {
  if (dtype != GCRNN_F32 && dtype != GCRNN_F64 && dtype != GCRNN_BF16) return 0;
  if (E != 1 || N <= 0 || N > GFL_MAX_N || nnz < 0 || nnz > N * N || F_in <= 0 || F_out <= 0 || K <= 0) return 0;
  if (F_in > 4096 || F_out > 4096 || K > 64) return 0;
  return gfl_lds(dtype, N, nnz, F_in, F_out, K, uniform) <= GFL_LDS_BYTES ? 1 : 0;
}

// one workgroup per slot: as many as fit on the chip at once (LDS-bound, at most 4 per CU), never more than there are items
extern "C" int64_t gcrnn_graph_filter_layer_wgrad_slots(int dtype, int64_t items, int64_t N, int64_t nnz, int64_t F_in, int64_t F_out,
                                                        int64_t K, int uniform) {
  if (items <= 0) return 0;
  const int64_t lds = gfl_lds(dtype, N > 0 ? N : 1, nnz > 0 ? nnz : 0, F_in > 0 ? F_in : 1, F_out > 0 ? F_out : 1, K > 0 ? K : 1, uniform);
  int64_t per_cu = lds > 0 ? GFL_LDS_BYTES / lds : 4;
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 4) per_cu = 4;
  const int64_t slots = GFL_CUS * per_cu;
  return items < slots ? items : slots;
}

// ---- plain RNN (gcrnn_rnn.hip): envelope and slot count from rnn_layout, host logic only ------------------------------------------
extern "C" int gcrnn_rnn_supported(int dtype, int64_t B, int64_t T, int64_t D, int64_t F_h) {
  if (dtype != GCRNN_F32 && dtype != GCRNN_F64) return 0;
  return rnn_layout(B, T, D, F_h).ok;
}

extern "C" int64_t gcrnn_rnn_wgrad_slots(int dtype, int64_t B, int64_t T, int64_t D, int64_t F_h) {
  if (!gcrnn_rnn_supported(dtype, B, T, D, F_h)) return 0;
  return rnn_layout(B, T, D, F_h).slots;
}
