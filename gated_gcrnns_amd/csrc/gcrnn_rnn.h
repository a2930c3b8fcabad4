// Envelope and launch geometry of the plain-RNN kernels (gcrnn_rnn.hip), shared with the host-side queries (gcrnn_host.cpp) so
// that the `supported` answer, the slot count and the launches agree.
#pragma once
#include <stdint.h>

constexpr int64_t RNN_MAX_FH = 64;                 // one wave per sequence: lane j owns hidden unit j and row / column j of W_hh
constexpr int64_t RNN_MAX_D = 65536;               // input width N*F_i (the projection streams it; nothing of it stays on chip)
constexpr int64_t RNN_MAX_ELEMS = (int64_t)1 << 31;  // B*T*(D + F_h + 1) and every tensor of the pass below 2^31 elements
constexpr int64_t RNN_COLS_TILE = 64;              // weight-gradient columns per workgroup
constexpr int64_t RNN_SLOT_ROWS = 64;              // at least this many (b, t) rows per weight-gradient slot
constexpr int64_t RNN_MAX_SLOTS = 64;              // slot count: a function of B*T alone (deterministic on every device)

struct RnnLayout {
  int ok;          // 1: the kernels evaluate this shape
  int fh_pad;      // W_hh row / column length held in registers: 4, 8, 16, 32 or 64
  int64_t rows;    // B*T
  int64_t cols;    // weight-gradient columns: D (W_ih), F_h (W_hh), 1 (the biases)
  int64_t col_tiles, slots, rows_per_slot;
};

static inline RnnLayout rnn_layout(int64_t B, int64_t T, int64_t D, int64_t Fh) {
  RnnLayout L{};
  if (B <= 0 || T <= 0 || D <= 0 || Fh <= 0 || Fh > RNN_MAX_FH || D > RNN_MAX_D) return L;
  if (B > RNN_MAX_ELEMS || T > RNN_MAX_ELEMS) return L;
  L.rows = B * T;
  L.cols = D + Fh + 1;
  if (L.rows > RNN_MAX_ELEMS / L.cols) return L;
  L.fh_pad = Fh <= 4 ? 4 : Fh <= 8 ? 8 : Fh <= 16 ? 16 : Fh <= 32 ? 32 : 64;
  L.col_tiles = (L.cols + RNN_COLS_TILE - 1) / RNN_COLS_TILE;
  int64_t s = (L.rows + RNN_SLOT_ROWS - 1) / RNN_SLOT_ROWS;
  L.slots = s < RNN_MAX_SLOTS ? s : RNN_MAX_SLOTS;
  L.rows_per_slot = (L.rows + L.slots - 1) / L.slots;
  L.ok = 1;
  return L;
}
