// Sequence-resident fused GCRNN recurrence, 32-feature chunks (round 4): the flagship forward of uniform-weight graphs.
//
// gcrnn_fused_seq.h keeps a sequence's operand [h_{t-1} | x_t] in registers and walks its F/16 output chunks; its phase stamps said
// (DESIGN 4.0): a hop stream costs ~1,150 fixed cycles + 73 per trip for ONE wave whatever the other waves do, the tap MFMAs and
// the acc = tap + w * sum FMAs follow strictly behind it, every chunk ends in a barrier-separated epilogue, and every step waits
// ~100 units for the operand it has just stored to come back from L2. This kernel changes what a hop processes:
//  * 32 output features per chunk as TWO 16-feature image planes (plane 1 = plane 0 + GCRNN_HOP_WIDE_PLANE bytes) read by ONE stream:
//    one column read and two address XORs per trip serve four 16-byte gathers and two v_smfmac (GCRNN_HOP_ASM_WIDE32_TEXT,
//    tools/gen_hop_asm.py gen_wide32) -- half the streams, barriers, seeds and epilogues per step, the per-trip overhead amortised
//    over twice the bytes. Plan arrays are those of the 16-feature bf16 image (graph.fused_plan_img16) unchanged.
//  * the graph weight w is folded into the tap weights (W_k <- w^k W_k, gcrnn_fused_pack_weights_wide): Horner then reads
//    t_j = u~_j + P0 t_{j+1} on the 0/1 pattern P0, so a hop's sums need no multiply and the tap MFMAs accumulate straight ONTO them
//    (D = A B + D): no separate tap tuple, no packed FMAs -- the registers that frees hold the second half's accumulators.
//  * output features are assigned to MFMA rows so that lane (r, q) ends a chunk holding features 32 c + 8 q .. + 7 of its node
//    (half h, row 4 q + e <-> feature 32 c + 8 q + 4 h + e; a permutation of the weight rows only): ONE 16-byte state store per lane
//    and tile -- and those four packed registers ARE the lane's B fragment of k-step c for the next time step. The last chunk's state
//    is handed over in registers; the earlier chunks' (stored long before) and x_{t+1} are requested at the start of the last
//    chunk's epilogue, so the step boundary waits for nothing that was not already on its way.
//  * LDS: planes / transposed user-layout tile 66 KB | ONE chunk's weight fragments K*KS*2 KB (the next chunk's arrive by LDS-DMA
//    during the epilogue) | column words | a 128-node inline-pack tile (8 rounds per step, one per hop at K = 5).
//    At START-UP (self-start, VAR 7 or 13 with Seq32Args::self_start; before the tables, the weights and the first seed): bytes [0, 64 KB) -- the
//    two planes, below the bias table -- are a staging area of 32 feature rows x 1024 nodes x 2 B (pitch 2 KB, the 16-byte pieces of row R
//    rotated by 2 (R >> 3) places) that whole 32-feature k-steps of the USER-layout h0 and x_0 pass through on their way into the operand
//    registers, then G rows x RPH * 128 nodes of x_1 on their way into the sequence-major work buffer.
// Arithmetic differs from the 16-feature kernels only in rounding (w^k W_k rounded to bf16 instead of W_k, sums before taps), so this
// kernel is pinned to the fp64 oracle directly (tests/test_fused.py), not bit-compared with them.
//
// MODE 0: forward step h_t = tanh(sum_k S^k([h|x] W_k) + 2b)   (reference Utils/graphML.py:2420-2423), un-gated.
#pragma once

// In-kernel phase stamps (diagnostic builds only, -DGCRNN_SEQ_STAMPS; tools/seq32_stamps.py): lane 0 of wave 0 records s_memtime at its
// phase boundaries of ONE step into LDS (FLAG_OFF, no scalar registers held), copied out at the end.
#if defined(GCRNN_SEQ_STAMPS)
static __device__ unsigned long long gcrnn_seq32_stamps[256 * 96];
// (explicit LDS instructions: a generic-pointer volatile access of the dynamic LDS array makes hipcc emit an illegal compare in some instantiations)
static __device__ __forceinline__ void gcrnn_stamp32_put(uint32_t lds_addr) {
  const unsigned long long tv = __builtin_amdgcn_s_memtime();
  asm volatile("ds_write_b64 %0, %1" ::"v"(lds_addr), "v"(tv) : "memory");
}
static __device__ __forceinline__ unsigned long long gcrnn_stamp32_get(uint32_t lds_addr) {
  unsigned long long tv;
  asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(tv) : "v"(lds_addr) : "memory");
  return tv;
}
#define GCRNN_STAMP32(slot)                                                                                   \
  do {                                                                                                        \
    if (wave == 0 && stamp_on && lane_now() == 0) gcrnn_stamp32_put((uint32_t)reinterpret_cast<uintptr_t>(smem) + M::FLAG_OFF + 8 * (slot)); \
  } while (0)
#define GCRNN_STAMP32_WAVE(slot0)                                                                             \
  do {                                                                                                        \
    if (stamp_on && lane_now() == 0) gcrnn_stamp32_put((uint32_t)reinterpret_cast<uintptr_t>(smem) + M::FLAG_OFF + 8 * ((slot0) + wave)); \
  } while (0)
#define GCRNN_STAMP32_FLUSH()                                                                                 \
  do {                                                                                                        \
    __syncthreads();                                                                                          \
    if (threadIdx.x < 96 && blockIdx.x < 256) gcrnn_seq32_stamps[blockIdx.x * 96 + threadIdx.x] = gcrnn_stamp32_get((uint32_t)reinterpret_cast<uintptr_t>(smem) + M::FLAG_OFF + 8 * threadIdx.x); \
  } while (0)
#ifndef GCRNN_SEQ32_STAMP_READER_NAME
#define GCRNN_SEQ32_STAMP_READER_NAME gcrnn_debug_read_seq32_stamps      // (one reader per translation unit that includes this header: gcrnn_fused_seq32p.hip names its own)
#endif
extern "C" int GCRNN_SEQ32_STAMP_READER_NAME(void* host) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(gcrnn_seq32_stamps), sizeof(unsigned long long) * 256 * 96) == hipSuccess ? 0 : 1;
}
#else
#define GCRNN_STAMP32_WAVE(slot0) do {} while (0)
#define GCRNN_STAMP32(slot) do {} while (0)
#define GCRNN_STAMP32_FLUSH() do {} while (0)
#endif

#ifndef GCRNN_SEQ32_R1_STREAM_FIRST
#define GCRNN_SEQ32_R1_STREAM_FIRST 0      // 1 (with R1): every wave streams first, as round 4's first rank-1 variant did (A/B)
#endif
#ifndef GCRNN_SEQ32_OPERAND_AT
#define GCRNN_SEQ32_OPERAND_AT 1      // where the last chunk requests the next step's operand: 0 = at the start of its epilogue, 1 = behind its state stores, 2 = behind its row stores (A/B)
#endif
// cache policy experiments (aux bits of the buffer / LDS-DMA instructions: 2 = nt): traffic this launch never reads again should not
// displace from L2 what it reads back one step later (x_{t+1} laid out by the pack, h_t's first chunk)
#ifndef GCRNN_SEQ32_NT_ROWS
#define GCRNN_SEQ32_NT_ROWS 0      // user-layout row stores
#endif
#ifndef GCRNN_SEQ32_NT_DMA
#define GCRNN_SEQ32_NT_DMA 0       // LDS-DMA reads of the user-layout input
#endif
#ifndef GCRNN_SEQ32_NT_XLOAD
#define GCRNN_SEQ32_NT_XLOAD 0     // requests of the next operand (read once)
#endif
#ifndef GCRNN_SEQ32_NT_STATE
#define GCRNN_SEQ32_NT_STATE 0     // state stores of the LAST chunk (handed over in registers: not read back by this launch)
#endif
#ifndef GCRNN_SEQ32_NO_ITEM_PREFETCH
#define GCRNN_SEQ32_NO_ITEM_PREFETCH 0      // 1: the gate pre-pass loads every item's operand at the item's start (A/B)
#endif
#ifndef GCRNN_SEQ32_GATED_TAPS_FIRST
#define GCRNN_SEQ32_GATED_TAPS_FIRST 1      // 1 (default): in the time-gated recurrence EVERY wave evaluates the tap before its stream (exact, no reciprocal).
                                            // 0: waves 0..3 stream first and start the gated chain from S / gf -- built, but hipcc then spills 4-8 operand registers
                                            // in the K = 4, 5 instantiations (the extra scaling pass keeps a reciprocal live across the MFMA chains): not the default
#endif
#ifndef GCRNN_SEQ32_YOUNG_PRIO
#define GCRNN_SEQ32_YOUNG_PRIO 0
#endif
#ifndef GCRNN_SEQ32_END_WAIT
#define GCRNN_SEQ32_END_WAIT 0     // 1: every chunk ends with s_waitcnt vmcnt(0) (as the first versions did; A/B)
#endif
#ifndef GCRNN_SEQ32_SAME_ORDER
#define GCRNN_SEQ32_SAME_ORDER 0      // 1: every wave streams first, then evaluates the tap (A/B: tools/ab_build.sh "-DGCRNN_SEQ32_SAME_ORDER=1")
#endif

struct Seq32Args {
  const uint16_t* x0; int64_t xstride;                 // x of step 0 [B][NP][G] bf16 sequence-major, elements between steps
  const uint16_t* hfirst;                              // h_{-1} = h0 [B][NP][F]
  uint16_t* out0; int64_t ostride;                     // h_t of step 0 [B][NP][F], elements between steps
  const uint4* wpack;                                  // [F/32][K][2][KS][64] x 16 B (gcrnn_fused_pack_weights_wide)
  const float* bias;                                   // [F] or null
  const uint16_t* a1; int64_t a1stride;                // user-layout output H[0][t] (or null)
  int a1_last_only;                                    // only the last step writes the user-layout output (at a1 itself)
  int ubstride;                                        // elements between consecutive sequences of the user-layout output
  const int32_t* tile_nodes; const int32_t* tile_off; const uint2* ell_col4;      // bf16-image plan (graph.fused_plan_img16)
  int entries, B, N;
  const uint16_t* pk_src0; int64_t pksrc_stride;       // inline pack: user-layout block X[0][0] (or null), elements between steps
  uint16_t* pk_dst0; int64_t pkdst_stride;             // ... the sequence-major array of step 0, elements between steps
  int pk_stride;                                       // ... elements between consecutive sequences of the user-layout tensor
  int nsteps;
  // GATED (time-gated recurrence, graphML.py:2357-2374, 2420-2421): scalar gates of step 0 [B] fp32, elements between steps
  const float* gi0; const float* gf0; int64_t gstride;
  // MODE 1 (gate-PAIR pre-pass: both time gates' sub-cells of every (t, b) item in one pass, graphML.py:2362-2374):
  int hmod;                                            // item i reads the state operand of sequence i % hmod (its h0)
  const int32_t* flags;                                // (or null) flags[0] != 0: h0 is all zeros -- the state half is neither loaded nor multiplied
  const float* gw;                                     // read-out weights of the two gates, [2][N][F] fp32 (node-major)
  const uint4* tapf; float* taps_out; int ntaps;       // MODE 1 (or null; then gw is unused): NODE gates (graphML.py:2379-2393) -- the gate cells' F -> 1 filters, taps first
                                                       // (:2387): A fragments [2 gates][F/32][3 planes][64 lanes] x 16 B of their taps (p0 + p1 + p2 = w to 24 bits; lane
                                                       // 16 kg + tap: w_p[tap][32 cg + 8 kg .. + 7]), output [items][2][F/32][ntaps][N] fp32 partial dots per chunk
  float* go;                                           // [items][2 * F/32 * 8] partial dot products per (chunk, wave); chunks 0 .. F/32-1 = input gate
  uint16_t* out1;                                      // (or null, with out0) the forget gate cell's states [items][NP][F]; out0 = the input gate cell's
  // MODE 2 (BPTT data chain, the adjoint of graphML.py:2420-2423): step i walks t = T-1-i; operand dpre_t = hfirst (step 0) / the previous
  // step's output, output dpre_{t-1} = out0 + i ostride; epilogue operands of step i (negative strides walk backwards in time):
  const uint16_t* dh0_; int64_t dhstride;              // upstream gradient dH_{t-1} [B][NP][F] sequence-major
  const uint16_t* hs0; int64_t hsstride;               // state h_{t-1}
  const float* gsc0; int64_t gscstride;                // (or null) forget gates gf_t [B] of the time-gated cell
  float* gpart0; int64_t gpartstride;                  // (or null) [B][F/32 * 8] partials of <h_{t-1}, adjoint chain of dpre_t> (the forget gate's gradient)
  int final_raw;                                       // != 0: the launch's LAST step stores the raw state gradient (d h0: no upstream term, no tanh') into
  uint16_t* final_out; const uint16_t* final_h;        // final_out (or null), with final_h (h0, or null) as the state of its partials
  // MODE 3 (filter-output pass, graphML.py:2402-2403: A(S) x_t + b for every (t, b) item; operand [0 | x_t], the state half never loaded): out0
  // [items][NP][F] bf16 receives acc + b (no activation). MODE 4 (node-gated recurrence, graphML.py:2379-2407, 2420-2423): state-only operand,
  // h_t = tanh(gi ni_t . Yx_t + gf nf_t . (B(S) h_{t-1} + b)) -- Yx_t = dh0_ + step dhstride (MODE 3's output), the per-node gates:
  const float* ng0; int64_t ngstride; int64_t nghalf;  // ng0 + step ngstride: ni [B][N] fp32, nf = + nghalf; optional scalar time gates gi0 / gf0 (+ step gstride)
  const float* r1a; const float* r1b;                  // R1 (rank-1-weighted graph S[m][n] = a[m] b[n], plan of its 0/1 pattern): the factors [NP] fp32, zero for padding rows
  int stagger;                                         // > 0: workgroup i starts ((i / 8) % 8) * stagger shader cycles late (de-synchronises the CUs' memory phases for the whole launch)
  uint16_t* scr;                                       // VAR bit 2: the state scratch [workgroups][HS-1][NP slots][32] bf16 (out0 is null: no state image)
  // VAR bit 3 (output head Linear(F -> 1) shared by all nodes, evaluated on the packed state in the epilogue; no user-layout output):
  const float* head_w; const float* head_b;            // [F] fp32, one fp32 on the device (or null)
  float* y0;                                           // y [B][nsteps][N] fp32
  // Self-start (VAR 7 and 13, MODE 0, un-gated; wave-uniform runtime switch: the code sits outside the step loop): the first operand
  // [h0 | x_0] of a sequence comes from the USER-layout tensors h0u [B][F][N] and pk_src0 (X[b][0]); step 0 lays out x_1. x0 / pk_dst0 is
  // then a work buffer of this launch (slot 0 is never touched), hfirst is not read.
  const uint16_t* h0u; int self_start;
  // VAR bit 4 (MODE 2, rank-1 upstream: the loss reaches the states through an output head Linear(F -> 1) shared by all nodes, so
  // dH_t[f][n] = head_w[f] dy_t[n] is never materialised): dy0 = dy[0][t] of chain step 0 in the USER layout [B][T][N] bf16, elements between
  // steps (negative: backwards in time) and between sequences; head_w [F] fp32 as above. dh0_ and the pack arguments are unused.
  const uint16_t* dy0; int64_t dystride; int64_t dybstride;
};

// this lane's id, re-derived where it is needed (two VALU instructions; volatile: neither hoisted nor kept): anything derived from the
// thread id that lives across a hop's asm block costs a register the operand, the accumulators and the stream's window do not leave
__device__ __forceinline__ int lane_now() {
  int ln;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
  return ln;
}

// (the stream ADDS the gathered rows to D: the caller zeroes D, or has already put the hop's tap there)
#define GCRNN_HOP_ASM_WIDE32_STREAM(D)                                                             \
  do {                                                                                             \
    const int gwbeg = tbeg[0] >> 2, gwend = tend[STILES - 1] >> 2;                                 \
    if (gwbeg < gwend) {                                                                           \
      const int ls_ = lane_now(), r = ls_ & 15, q = ls_ >> 4;                                      \
      const uint32_t colb = lds_col + r * 8 + (q >> 1) * 4;       /* this lane's own column dword of a slot's pair */ \
      const uint32_t qh_ = (uint32_t)(q & 1) << 4;                                                 \
      asm volatile(GCRNN_HOP_ASM_WIDE32_TEXT                                                       \
                   : "+v"(D[0][0]), "+v"(D[0][1]), "+v"(D[1][0]), "+v"(D[1][1]), "+v"(D[2][0]), "+v"(D[2][1]), "+v"(D[3][0]), "+v"(D[3][1]), \
                     "+v"(D[4][0]), "+v"(D[4][1]), "+v"(D[5][0]), "+v"(D[5][1]), "+v"(D[6][0]), "+v"(D[6][1]), "+v"(D[7][0]), "+v"(D[7][1])  \
                   : "s"(GCRNN_SGPR(tend[0] >> 2)), "s"(GCRNN_SGPR(tend[1] >> 2)), "s"(GCRNN_SGPR(tend[2] >> 2)), "s"(GCRNN_SGPR(tend[3] >> 2)), \
                     "s"(GCRNN_SGPR(tend[4] >> 2)), "s"(GCRNN_SGPR(tend[5] >> 2)), "s"(GCRNN_SGPR(tend[6] >> 2)), "s"(GCRNN_SGPR(tend[7] >> 2)), \
                     "s"(GCRNN_SGPR(gwbeg)), "s"(GCRNN_SGPR(gwend - 1)), "v"(colb), "v"(qh_)               \
                   : GCRNN_HOP_ASM_WIDE32_CLOBBERS);                                               \
    }                                                                                              \
  } while (0)

// RT > 0 (resident tiles; the un-gated self-start forward with more than one chunk): the weight fragments live in a RING of three taps
// instead of a whole chunk's K -- a hop reads ONE tap, and the taps are consumed in a fixed order (chunk 0: tap K-1 .. 0, chunk 1: tap
// K-1 .. 0, the next step ...), so item g of that order sits in slot g % 3 and arrives by LDS-DMA two hops before it is read. Behind the
// ring, in the bytes it frees, lies a block of RT tiles per wave and re-read chunk: [HS-1][SWAVES][RT] x 1 KB, lane-linear (16 bytes per
// lane), where a wave keeps the state fragments of its first RT tiles between the epilogue that makes them and the next step's operand
// instead of sending them through the state scratch. At K = 5, F = G = 64: 24 KB ring + 16 KB block = the 40 KB of today's WB.
template <int K, int HS, int XS, int RT = 0>
struct Seq32Map {
  static constexpr int KS = HS + XS;
  static constexpr int PL = GCRNN_HOP_WIDE_PLANE;          // plane 1 of the hop image
  static constexpr int RS2 = 4 * NP + 16;                  // row of the transposed user-layout tile: [feature pair][node] words; q and q + 1 sit 16 banks apart
  static constexpr int BIAS_OFF = PL + 32 * 1024;          // behind plane 1 (the transposed tile, 16 rows, ends below it)
  static constexpr int FLAG_OFF = BIAS_OFF + 256;
  static constexpr int WOFF = 2 * PL;                      // the weight fragments: one chunk's, or the ring
  static constexpr int RING = RT > 0 ? 3 : K;              // taps held in LDS
  static constexpr int TAPB = KS * 2048;                   // one tap's fragments: 2 KS pieces of 1 KB
  static constexpr int WCH = K * TAPB;                     // one chunk's fragments in the packed weights (global memory)
  static constexpr int WB = RING * TAPB;
  static constexpr int RES_OFF = WOFF + WB;                // resident tiles: wave-private, lane-linear
  static constexpr int RES_B = RT * (HS - 1) * SWAVES * 1024;
  static constexpr int COL_OFF = RES_OFF + RES_B;
  static constexpr int NPCK = 128;                         // nodes per inline-pack round
  static constexpr int PFS = 256;                          // prefetch scratch (one dword per lane)
  static_assert(16 * RS2 <= BIAS_OFF && FLAG_OFF + 768 <= WOFF, "LDS map");
  static_assert(RT >= 0 && RT <= STILES && (RT == 0 || HS > 1), "resident tiles: a share of a wave's tiles, of a state with a re-read chunk");
  // planes / transposed tile, bias and flag tables < WOFF <= ring < RES_OFF <= block < COL_OFF <= column words, slot table, (rank-1
  // factors, head table,) pack tile, PFS: lds_bytes() lays those out upwards from COL_OFF, so nothing overlaps the block
  static_assert(WOFF + RING * TAPB == RES_OFF && RES_OFF + RES_B == COL_OFF && RES_OFF % 1024 == 0, "LDS map: ring, resident block, column words");
  static size_t lds_bytes(int64_t entries, bool inline_pack, bool r1 = false) {
    const size_t need = (size_t)COL_OFF + (size_t)entries * 32 + GCRNN_HOP_COLUMN_PAD + NP * 4 + (r1 ? 2 * NP * 4 : 0) + (inline_pack ? (size_t)(32 * (XS > 0 ? XS : HS)) * NPCK * 2 : 0)
                        + PFS;      // (the last PFS bytes: where gcrnn_fused_seq32p.h's L2 prefetches land -- LDS-DMA needs a destination, nobody reads it)
    return need <= 160 * 1024 ? need : 0;
  }
  // VAR bit 3: the head's table in front of the inline-pack tile -- F weights, the bias at [64], and (HS > 1) one partial sum per slot
  static constexpr int HEAD_TAB = 512 + (HS > 1 ? NP * 4 : 0);
  static size_t lds_bytes_head(int64_t entries, bool inline_pack, bool r1 = false) {
    const size_t need = lds_bytes(entries, inline_pack, r1);
    return (need && need + HEAD_TAB <= 160 * 1024) ? need + HEAD_TAB : 0;
  }
};

// VAR: bit 0 = the launch lays out the input itself (inline pack), bit 1 = it writes the user-layout output. Compile-time so that every way
// the forward is issued -- as the module issues it (3), caller-packed X (2), sequence-major in and out (0) -- is a kernel symbol of its own in a
// trace (profiles/*kernel_stats.csv reproduce the bench line's roofline fraction), and the paths not taken cost neither code nor registers.
// Bit 2 (with bit 1, MODE 0, persistent form: inference, where H leaves through the user-layout tile and nobody reads the sequence-major state
// image): no state image at all. The only state bytes this launch reads back are chunks 0 .. HS-2 of h_t, one step later (chunk HS-1 is handed
// over in registers): they go to a scratch of this WORKGROUP, [HS-1][NP][32] bf16 in SLOT order (row = (wave * STILES + tile) * 16 + r), so a
// wave-instruction stores -- and later loads -- 1 KB of contiguous bytes instead of sixteen half-used 128-byte lines of [node][F] rows, and
// neither side needs the slot table. Chunk HS-1 is not stored to memory (at HS = 1 nothing is stored or reloaded); step 0 reads h0 as before.
// ONE buffer for all steps and sequences of the workgroup: a lane reloads exactly the 16 bytes it stored itself. In its program order the
// reload of step t (requested in the last chunk's epilogue) has been consumed by the seed's MFMAs of step t+1 -- which wait for it -- before
// chunk 0's epilogue of step t+1 stores to the address again, and that store has retired behind the vmcnt(0) of every later hop before the
// next reload is requested. The addresses are re-used every step, so the reload carries sc1: it is served by L2 (where the line comes from
// anyway, a step after its store) whatever this CU's vector L1 still holds of the previous step's line.
// Bit 3 (with bit 2, without bit 1; MODE 0, persistent form: inference of cell + output head Linear(F -> 1) shared by all nodes): no state
// image and no user-layout output either. The state hand-over is bit 2's; the epilogue adds y_t[n] = b + sum_f w[f] bf16(h_t[n][f]) on the
// packed registers it holds anyway -- eight FMAs per lane and tile in feature order, the four quads of a node by two xor-shuffles (16, 32),
// the chunks in ascending order through one LDS word per slot that the same lane writes and reads (a lane keeps its slots in every chunk:
// slot = (wave * STILES + tile) * 16 + r) -- and the q == 0 lanes store the 4-byte results straight to y [B][T][N] (rows >= N never).
// Bit 4 (MODE 2 only, persistent form, uniform-weight graph; alone): rank-1 upstream gradient. The epilogue's operand dH_{t-1} of lane (node,
// 8 features) is head_w[f] * dy_{t-1}[node] rounded to bf16 -- the bits the head's backward kernel would have stored into dH -- made from ONE
// 16-bit load of dy in the user layout [B][T][N] (descriptor of the row: nodes >= N read 0) and the head's weights in the bias table's
// place in LDS (the chain has no bias). No sequence-major dH, no pack rounds; the requests sit where the dH requests sat.
// MODE 0: the recurrence (GATED: with the scalar time gates gi_t, gf_t known before step 0 -- they read (x_t, h0), never h_{t-1}).
// MODE 1: the time gates' pre-pass for BOTH gates at once: an item (t, b) is one "sequence" of one step whose cell has 2 F outputs -- chunks
//         0 .. F/32-1 the input gate's sub-cell, the rest the forget gate's (weights and biases concatenated by the caller) -- so the operand
//         (x_t, h0) is loaded, and with VAR bit 0 laid out, ONCE per gate pair; epilogue: c = tanh(pre), partial <c, read-out weights>.
// MODE 2: the BPTT data chain dpre_{t-1} = (gf_t sum_k S^k (dpre_t B_k^T) + dH_{t-1}) (1 - h_{t-1}^2) on the adjoint graph with the transposed
//         state taps: a state-only operand (XS = 0) that is entirely this launch's own output -- the last chunk handed over in registers,
//         the first re-read --, the epilogue's operands dH_{t-1}, h_{t-1} requested at the chunk's start; VAR bit 0: lays out dH.
// R1: rank-1-weighted graph S[m][n] = a[m] b[n] (normalised adjacencies: graph.fused_plan_rank1) on the plan of its 0/1 pattern: a hop is
//     b[n] sum_{m in N(n)} (a[m] v[m]) -- every image write is scaled by a (seed and hop outputs), a hop's sums by b BEFORE its tap is added
//     (so every wave streams first), the taps carry no w^k (uniform_w = 1).
// SPLIT: batches that leave half of the chip idle (65 <= B <= 128 at F = 64): a sequence's F/32 chunks run as F/32 WORKGROUPS, one launch per time
//     step (the launch boundary is the hand-over between them: no cross-workgroup wait inside a launch). Each loads the whole operand, runs its
//     chunk, stores its 32 features and lays out its share of the next step's input; nothing is kept in registers across steps.
// RT (Seq32Map; VAR 7 only, HS > 1): the tap ring, and the first RT tiles of every wave hand their chunks 0 .. HS-2 to the next step through
//     the wave-private LDS block instead of the state scratch. The block is written in step t and read in step t + 1 of the SAME workgroup
//     and sequence only (step 0 reads h0), so nothing carries over to a workgroup that runs on the CU afterwards, or to the next sequence of
//     a persistent workgroup. RT = 0: one chunk's K taps in LDS and every tile through the scratch, the kernel as it was.
template <int K, int HS, int XS, int VAR, int MODE = 0, bool GATED = false, bool R1 = false, bool SPLIT = false, int RT = 0>
__global__ __launch_bounds__(STHREADS) void fused_seq32_kernel(const Seq32Args a) {
  static_assert(!R1 || !SPLIT, "rank-1 graphs: every mode of the persistent form (the BPTT chain takes the adjoint plan: the factors swap)");
  static_assert(!SPLIT || ((MODE == 0 || MODE == 2) && !R1 && HS > 1), "split sequences: the (un-gated or time-gated) forward and the BPTT chain, with more than one chunk");
  constexpr bool ITEMS = (MODE == 1 || MODE == 3);      // one-step items (t, b) instead of sequences
  constexpr bool SONLY = (MODE == 2 || MODE == 4);      // state-only operand that is this launch's own output (XS = 0)
  constexpr bool PKV = (VAR & 1) != 0, USERV = (VAR & 2) != 0 && (MODE == 0 || MODE == 4);
  constexpr bool SCRV = (VAR & 4) != 0;      // state scratch in slot order, no state image
  constexpr bool HEADV = (VAR & 8) != 0;     // output head in the epilogue, y instead of H
  constexpr bool UPR1 = (VAR & 16) != 0;     // chain: the upstream gradient is head_w (x) dy, made in the epilogue
  static_assert(!UPR1 || (VAR == 16 && MODE == 2 && !R1 && !SPLIT), "rank-1 upstream: the persistent chain on uniform-weight graphs, no inline pack");
  static_assert(!SCRV || (MODE == 0 && !SPLIT && ((VAR & 2) != 0 || HEADV)), "state scratch: the persistent forward with the user-layout output");
  static_assert(!HEADV || (SCRV && (VAR & 2) == 0), "output head: on the state scratch, no user-layout output");
  constexpr int SCR_CH = NP * 64;            // bytes of one chunk's scratch rows [NP slots][32] bf16
  static_assert(MODE == 0 || ((MODE >= 1 && MODE <= 4) && !GATED), "modes");
  static_assert(MODE < 3 || (!R1 && !SPLIT), "modes 3, 4: uniform-weight graphs, persistent form");
  using M = Seq32Map<K, HS, XS, RT>;
  constexpr bool RINGV = RT > 0;
  static_assert(!RINGV || (VAR == 7 && MODE == 0 && !GATED && !SPLIT && HS > 1), "resident tiles: the un-gated self-start forward, more than one chunk");
  constexpr int KS = HS + XS;
  constexpr int F = 32 * HS, G = 32 * XS;
  constexpr int NCH = (MODE == 1) ? 2 * HS : HS;  // 32-feature output chunks
  constexpr int PL = M::PL, WOFF = M::WOFF, WCH = M::WCH, TAPB = M::TAPB, COL_OFF = M::COL_OFF, RS2 = M::RS2;
  constexpr int NPCK = M::NPCK, NRND = NP / NPCK, NH = NCH * (K - 1), RPH = (NRND + NH - 1) / NH;      // pack rounds per step / hops per step / rounds per hop
  constexpr int PKROWS = SONLY ? F : G;
  static_assert(STILES == 8 && GCRNN_HOP_ASM && K >= 2 && (SONLY ? XS == 0 : XS > 0), "generated hop stream: 8 tiles per wave; the chain's operand is the state alone");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int entries = a.entries, B = a.B, N = a.N;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  constexpr int NSPL = SPLIT ? HS : 1;
  const int wg_seq = (int)blockIdx.x / NSPL, chunk0 = SPLIT ? (int)blockIdx.x % NSPL : 0, gseq = (int)gridDim.x / NSPL;
  if (wg_seq >= B) return;

  bf16x8 bfr[STILES][KS];      // the operand of a sequence and step: every B fragment of the wave, resident for all chunks
  // Self-start (ONE sequence per workgroup: the host launches B workgroups, so this IS the top of every sequence and the loop below runs
  // once -- beyond one workgroup per CU they start as CUs free up, which is the order the persistent loop walks them in): the operand [h0 | x_0] from the USER layout (h0 [B][F][N],
  // X[b][0] [G][N]: rows = features), one 32-feature k-step at a time through the two hop-image planes, idle until the first seed: 32 rows x
  // NP nodes x 2 B = 64 KB below BIAS_OFF, ALL pieces of a k-step in flight per wave (8 x 16 B per lane), one vmcnt(0), a barrier -- then
  // lane (r, q) of tile i picks features 32 s + 8 q .. + 7 of its slot's node out of rows 8 q .. 8 q + 7, which IS bfr[i][s]: no global
  // round trip. The 16-byte pieces of row R sit rotated by 2 (R >> 3) places (by the SOURCE address: an LDS-DMA destination is
  // lane-linear), so the four quads of a wave -- rows 8 apart, 2 KB pitch = the same banks -- read bank groups 8 dwords apart. Columns
  // >= N are not fetched and rows >= N read as zeros, exactly what the caller's pack wrote. It runs FIRST, in front of the tile tables and
  // the launch's own LDS-DMA (which land above WOFF): here next to no scalar register is live yet -- at the top of the sequence loop every
  // scalar this code uses was one more spill lane of a kernel that sits at 255 vector registers.
  constexpr bool SELFV = PKV && SCRV && MODE == 0 && !GATED && !SPLIT;      // (VAR 7 and 13: the un-gated inference forward and its output-head form, uniform-weight or rank-1)
  const bool self_start = SELFV && a.self_start != 0;      // (wave-uniform: a kernel argument)
  if constexpr (SELFV) {
    if (self_start) {
      constexpr int SROW = NP * 2, SPIECES = 32 * (NP / 8);      // bytes per staged feature row, 16-byte pieces per k-step
      static_assert(32 * SROW <= M::BIAS_OFF && 32 * SROW <= M::WOFF && SPIECES % STHREADS == 0 && NP / 8 == 128, "self-start staging area: below the bias table");
      const int b = wg_seq;
      const int tl = wave * 64 + lane_now();
      int nodes[STILES];      // this lane's slot nodes (the slot table is not in LDS yet)
#pragma unroll
      for (int i = 0; i < STILES; ++i) nodes[i] = a.tile_nodes[(wave * STILES + i) * 16 + (tl & 15)] >> 16;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const uint16_t* src = s < HS ? a.h0u + (int64_t)b * (F * N) + (int64_t)(32 * s) * N
                                     : a.pk_src0 + (int64_t)b * a.pk_stride + (int64_t)(32 * (s - HS)) * N;
#pragma unroll
        for (int i = 0; i < SPIECES / STHREADS; ++i) {
          const int id = i * STHREADS + tl;
          const int row = id >> 7, cs = id & 127;
          const int col = (cs - 2 * (row >> 3)) & 127;
          if (col * 8 < N)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (int64_t)row * N + col * 8),
                                             (__attribute__((address_space(3))) void*)(smem + (i * STHREADS + wave * 64) * 16), 16, 0, GCRNN_SEQ32_NT_DMA);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();      // every wave's pieces of the k-step are in
        const int qo = (tl & 63) >> 4;
#pragma unroll
        for (int i = 0; i < STILES; ++i) {
          const bool ok = nodes[i] < N;
          const int nn = ok ? nodes[i] : 0;
          const char* ra = smem + (8 * qo) * SROW + ((((nn >> 3) + 2 * qo) & 127) << 4) + (nn & 7) * 2;
          uint32_t h16[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) h16[j] = *reinterpret_cast<const uint16_t*>(ra + j * SROW);
          typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int u32x4s_t;
          u32x4s_t v;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) v[jj] = ok ? (h16[2 * jj] | (h16[2 * jj + 1] << 16)) : 0u;
          bfr[i][s] = __builtin_bit_cast(bf16x8, v);
        }
        lds_barrier();      // the area is read: the next k-step's pieces may overwrite it
      }
      // x_1: step 0's ordinary pack rounds lay out rounds >= RPH of it (pack_target), shifted by one hop as in every step; the first RPH
      // rounds -- nodes [0, RPH * 128), which no hop of step 0 reaches -- are laid out here, through the same area: G rows x XN nodes, rotated
      // as above, then one 16-byte piece (node, 8 features) per lane and trip, the bytes pack_drain writes. Stored before step 0's first hop,
      // and every hop waits (vmcnt(0) + barrier) before the step's last epilogue requests x_1.
      if (a.nsteps > 1) {
        constexpr int XN = RPH * NPCK, XROWS = G, XPPR = XN / 8, XPCS = XROWS / 8;
        static_assert(XROWS * XN * 2 <= 32 * SROW && (XROWS * XPPR) % STHREADS == 0 && (XPCS * XN) % STHREADS == 0 && XPPR >= 16, "x_1 start-up rounds");
        // (gfx950 store-data hazard, DESIGN 4.1: the stores take an immediate soffset -- the sequence is in the descriptor's base --, every piece
        //  of a pass sits in its own register tuple before the first store, and the tuples stay reserved until the stores have retired)
        const __amdgpu_buffer_rsrc_t rsrc_x1 = __builtin_amdgcn_make_buffer_rsrc(a.pk_dst0 + a.pkdst_stride + (int64_t)b * (NP * G), 0, NP * G * 2, 0x00020000);
        const uint16_t* src = a.pk_src0 + (int64_t)b * a.pk_stride + a.pksrc_stride;
#pragma unroll
        for (int i = 0; i < XROWS * XPPR / STHREADS; ++i) {
          const int id = i * STHREADS + tl;
          const int row = id / XPPR, cs = id - row * XPPR;
          const int col = (cs - 2 * (row >> 3) + XPPR) % XPPR;      // (RPH = 3 at K = 4, F = 32: no power of two)
          if (col * 8 < N)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (int64_t)row * N + col * 8),
                                             (__attribute__((address_space(3))) void*)(smem + (i * STHREADS + wave * 64) * 16), 16, 0, GCRNN_SEQ32_NT_DMA);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();
        constexpr int XRI = XPCS * XN / STHREADS;
        typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int u32x4x_t;
        u32x4x_t vv[XRI];
#pragma unroll
        for (int i = 0; i < XRI; ++i) {
          const int id = i * STHREADS + tl;
          const int nl = id / XPCS, pc = id - nl * XPCS;
          const char* ra = smem + (8 * pc) * (XN * 2) + ((((nl >> 3) + 2 * pc) % XPPR) << 4) + (nl & 7) * 2;
          uint32_t h16[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) h16[j] = *reinterpret_cast<const uint16_t*>(ra + j * (XN * 2));
          const bool ok = nl < N;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) vv[i][jj] = ok ? (h16[2 * jj] | (h16[2 * jj + 1] << 16)) : 0u;
        }
#pragma unroll
        for (int i = 0; i < XRI; ++i) asm volatile("" : "+v"(vv[i]));
#pragma unroll
        for (int i = 0; i < XRI; ++i) {
          const int id = i * STHREADS + tl;
          const int nl = id / XPCS, pc = id - nl * XPCS;
          __builtin_amdgcn_raw_buffer_store_b128(vv[i], rsrc_x1, nl * (G * 2) + pc * 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < XRI; ++i) asm volatile("" ::"v"(vv[i]));      // (reserved until here)
        lds_barrier();      // the area is read: the launch's tables and the seed may follow
      }
    }
  }

  // once per launch: tile tables, and -- by LDS-DMA, all pieces in flight together -- the column image and chunk 0's weights
  int tbeg[STILES], tend[STILES];
#pragma unroll
  for (int i = 0; i < STILES; ++i) {
    tbeg[i] = a.tile_off[wave * STILES + i];
    tend[i] = a.tile_off[wave * STILES + i + 1];
  }
  // slot table node << 16 | row16 << 5 | hswz << 4 of every tile slot, in LDS: a lane reads its slot's word where it needs it (eight
  // live registers would not survive the hops: operand 128 + accumulators 64 + the stream's window)
  char* wtab = smem + COL_OFF + entries * 32 + GCRNN_HOP_COLUMN_PAD;
  for (int idx = tid; idx < NP; idx += STHREADS) reinterpret_cast<int32_t*>(wtab)[idx] = a.tile_nodes[idx];
  [[maybe_unused]] float* r1tab = reinterpret_cast<float*>(wtab + NP * 4);      // R1: a then b, in SLOT order (slot = (wave * STILES + tile) * 16 + row: one read, no index)
  if constexpr (R1) {
    for (int idx = tid; idx < NP; idx += STHREADS) {
      const int nd = a.tile_nodes[idx] >> 16;
      r1tab[idx] = nd < NP ? a.r1a[nd] : 0.f;
      r1tab[NP + idx] = nd < NP ? a.r1b[nd] : 0.f;
    }
  }
  // (one asm statement: eight reads in flight, one wait; volatile so that the words are re-read at every use, not kept)
  auto slot_words = [&](int ln, int (&w)[STILES]) {
    const uint32_t ad = (uint32_t)(COL_OFF + entries * 32 + GCRNN_HOP_COLUMN_PAD) + (uint32_t)((wave * STILES * 16 + (ln & 15)) * 4);
    asm volatile("ds_read_b32 %0, %8\n\tds_read_b32 %1, %8 offset:64\n\tds_read_b32 %2, %8 offset:128\n\tds_read_b32 %3, %8 offset:192\n\t"
                 "ds_read_b32 %4, %8 offset:256\n\tds_read_b32 %5, %8 offset:320\n\tds_read_b32 %6, %8 offset:384\n\tds_read_b32 %7, %8 offset:448\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(w[4]), "=&v"(w[5]), "=&v"(w[6]), "=&v"(w[7])
                 : "v"(ad));
    const int lb = (((ln >> 4) >> 1) << 4) | (((ln >> 4) & 1) << 3);      // xor this lane's (half, piece)
#pragma unroll
    for (int i = 0; i < STILES; ++i) w[i] ^= lb;
  };
  // R1: the accumulators of this wave's tiles times a per-node factor -- kind 0: b, 1: 1 / b, 2: b (b = 0, a node without in-neighbours: 1 for
  // kinds 1 and 2). Four tiles at a time: the eight slot words at once cost registers some instantiations do not have.
  [[maybe_unused]] auto r1_scale = [&](f32x4 (&ac)[STILES][2], int kind) __attribute__((always_inline)) {
    if constexpr (R1) {
      const uint32_t ad = (uint32_t)(COL_OFF + entries * 32 + GCRNN_HOP_COLUMN_PAD + NP * 4 + NP * 4) + (uint32_t)((wave * STILES * 16 + (lane_now() & 15)) * 4);      // b, slot order
      constexpr int NB = (GATED || ITEMS || K == 4) ? 1 : 4;      // factors read at a time (the instantiations at the register limit take them one by one: a few hundred cycles per hop)
#pragma unroll
      for (int h4 = 0; h4 < STILES; h4 += NB) {
        float b4[NB];
        if constexpr (NB == 4)
          asm volatile("ds_read_b32 %0, %4\n\tds_read_b32 %1, %4 offset:64\n\tds_read_b32 %2, %4 offset:128\n\tds_read_b32 %3, %4 offset:192\n\t"
                       "s_waitcnt lgkmcnt(0)"
                       : "=&v"(b4[0]), "=&v"(b4[1]), "=&v"(b4[2]), "=&v"(b4[3])
                       : "v"(ad + (uint32_t)(h4 * 64)));
        else
          asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(b4[0]) : "v"(ad + (uint32_t)(h4 * 64)));
#pragma unroll
        for (int e = 0; e < NB; ++e) {
          const float bv = b4[e];
          const float f = kind == 0 ? bv : (bv == 0.f ? 1.f : (kind == 1 ? __builtin_amdgcn_rcpf(bv) : bv));
          ac[h4 + e][0] *= f; ac[h4 + e][1] *= f;
        }
      }
    }
  };

  // RT > 0: the ring at the top of a sequence -- items 0 and 1 of the order (chunk 0's taps K-1 and K-2) in slots 0 and 1; hop 1 brings items 2, 3
  [[maybe_unused]] auto ring_start = [&]() {
    const char* w0 = reinterpret_cast<const char*>(a.wpack);
    const int ln = lane_now();
    for (int p = wave; p < 2 * (TAPB / 1024); p += SWAVES) {
      const int item = p / (TAPB / 1024), piece = p - item * (TAPB / 1024);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(w0 + (K - 1 - item) * TAPB + piece * 1024 + ln * 16),
                                       (__attribute__((address_space(3))) void*)(smem + WOFF + p * 1024), 16, 0, 0);
    }
  };
  {
    const int cbytes = entries * 32;
    const char* csrc = reinterpret_cast<const char*>(a.ell_col4);
    for (int p = wave; p * 1024 < cbytes; p += SWAVES)
      if (p * 1024 + lane * 16 < cbytes)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(csrc + p * 1024 + lane * 16),
                                         (__attribute__((address_space(3))) void*)(smem + COL_OFF + p * 1024), 16, 0, 0);
    const char* wsrc = reinterpret_cast<const char*>(a.wpack) + (size_t)chunk0 * WCH;      // (SPLIT: this workgroup's chunk)
    if constexpr (RINGV) ring_start();
    else
    for (int p = wave; p < WCH / 1024; p += SWAVES)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc + p * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(smem + WOFF + p * 1024), 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  // zeros behind the column image: the stream's running column pointer is not clamped (GCRNN_HOP_COLUMN_PAD)
  if (tid < GCRNN_HOP_COLUMN_PAD / 4) reinterpret_cast<uint32_t*>(smem + COL_OFF + entries * 32)[tid] = 0u;
  float* lbias = reinterpret_cast<float*>(smem + M::BIAS_OFF);
  if constexpr (UPR1) {      // (the chain adds no bias: the table holds the head's weights)
    if (tid < F) lbias[tid] = a.head_w[tid];
  } else
  if (tid < NCH * 32) lbias[tid] = a.bias ? a.bias[tid] : 0.f;
  if constexpr (HEADV) {
    float* ht = reinterpret_cast<float*>(smem + COL_OFF + entries * 32 + GCRNN_HOP_COLUMN_PAD + NP * 4 + (R1 ? 2 * NP * 4 : 0));
    if (tid < F) ht[tid] = a.head_w[tid];
    if (tid == F) ht[64] = a.head_b ? a.head_b[0] : 0.f;
  }
  __syncthreads();

  if (a.stagger > 0) {
    // All 256 workgroups run the same phases at the same time, so the chip's HBM sees every CU's operand requests / state stores / row
    // stores as bursts (11 B per clock and CU when all ask at once: profiles/r04_seq32_stamps_*.txt). A one-time offset per group of
    // workgroups persists over all T steps of this launch (same code, same speed) and spreads those bursts over the step.
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    const unsigned long long d = (unsigned long long)((blockIdx.x >> 3) & 7) * (unsigned long long)a.stagger;
    while (__builtin_amdgcn_s_memtime() - t0 < d) __builtin_amdgcn_s_sleep(16);
  }
  const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>(smem);
  if (lds0 != 0) __builtin_trap();        // the asm stream forms gather addresses from column words: the image must sit at LDS address 0
  const uint32_t lds_col = lds0 + COL_OFF;
  [[maybe_unused]] float* htab = reinterpret_cast<float*>(wtab + NP * 4 + (R1 ? 2 * NP * 4 : 0));      // HEADV: w [F] | b at [64] | partial sums [NP slots] from [128]
  char* xtile = wtab + NP * 4 + (R1 ? 2 * NP * 4 : 0) + (HEADV ? M::HEAD_TAB : 0);

  // wave-uniform, as a scalar integer (a lane mask would also be parked in a vector register)
  const int skip_hi = __builtin_amdgcn_readfirstlane((MODE == 3 || (MODE == 1 && a.flags && a.flags[0] != 0)) ? 1 : 0);      // (MODE 3: the operand is [0 | x_t])
  const bool skip_h = skip_hi != 0;
  // ---- the operand of a sequence and step: every B fragment of the wave, resident for all chunks ----------------------------------
  // the operand of item / sequence `bb` (its first step): at the top of the loop, or -- MODE 1 -- requested behind the previous item's last state
  // stores, when the operand registers have just died (the items of the pre-pass are one step each: without it every item starts with a
  // wait for its whole operand)
  auto load_first_operand = [&](int b) {
    // (MODE 1 with an all-zero h0: a zero-length descriptor -- the loads return zeros and cost nothing)
    const __amdgpu_buffer_rsrc_t rsrc_h = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.hfirst), 0, skip_h ? 0 : (ITEMS ? a.hmod : B) * (NP * F * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.x0), 0, XS > 0 ? B * (NP * G * 2) : 0, 0x00020000);
    const int bh = ITEMS ? __builtin_amdgcn_readfirstlane(b % a.hmod) : b;
    const int ln0 = lane_now(), qo = ln0 >> 4;
    int sw[STILES];
    slot_words(ln0, sw);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int i = 0; i < STILES; ++i) {
        const int w = sw[i];
        if (s < HS)
          bfr[i][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_h, (w >> 16) * (F * 2) + 16 * qo + 64 * s, bh * (NP * F * 2), 0));
        else
          bfr[i][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (w >> 16) * (G * 2) + 16 * qo + 64 * (s - HS), b * (NP * G * 2), 0));
      }
    }
  };
  bool have_operand = self_start;      // (wave-uniform; self-start: the one sequence's operand is in the registers already)
  for (int b = wg_seq; b < B; b += gseq) {
  if constexpr (RINGV) {
    // a persistent workgroup's next sequence: the order starts over (the last step's hops brought items of a step that never ran; every
    // wave is behind the last epilogue's end barrier, so nobody reads the ring)
    if (b != wg_seq) {
      ring_start();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();
    }
  }
  if (!have_operand) load_first_operand(b);
  have_operand = false;
#pragma unroll 1
  for (int step = 0; step < a.nsteps; ++step) {
    const bool fin = (MODE == 2) && a.final_raw && step == a.nsteps - 1;      // (chain: the d h0 step)
    uint16_t* hout = fin ? a.final_out : (a.out0 ? a.out0 + (int64_t)step * a.ostride : nullptr);
    [[maybe_unused]] const uint16_t* ep_dh = (SONLY && !fin && a.dh0_) ? a.dh0_ + (int64_t)step * a.dhstride : nullptr;      // (MODE 4: Yx_t)
    [[maybe_unused]] const float* ep_ng = (MODE == 4) ? a.ng0 + (int64_t)step * a.ngstride : nullptr;
    [[maybe_unused]] const uint16_t* ep_h = (MODE == 2) ? (fin ? a.final_h : (a.hs0 ? a.hs0 + (int64_t)step * a.hsstride : nullptr)) : nullptr;
    [[maybe_unused]] const uint16_t* ep_dy = (UPR1 && !fin && a.dy0) ? a.dy0 + (int64_t)step * a.dystride + (int64_t)b * a.dybstride : nullptr;      // dy[b][t-1][:]
    [[maybe_unused]] const bool ep_up = UPR1 ? ep_dy != nullptr : ep_dh != nullptr;      // (MODE 2: this step has an upstream term)
    [[maybe_unused]] float* gpart = (MODE == 2 && a.gpart0) ? a.gpart0 + (int64_t)step * a.gpartstride : nullptr;
    [[maybe_unused]] float gsc = 1.f;
    if constexpr (MODE == 2) {
      if (a.gsc0) gsc = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.gsc0[(int64_t)step * a.gscstride + b])));
    }
    float gin = 1.f, gfo = 1.f, gratio = 1.f;
    if constexpr (MODE == 4) {      // scalar time gates on top of the node gates (applied in the epilogue)
      if (a.gi0) {
        gin = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.gi0[(int64_t)step * a.gstride + b])));
        gfo = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.gf0[(int64_t)step * a.gstride + b])));
      }
    }
    if constexpr (GATED) {      // (wave-uniform: kept in scalar registers -- three vector registers live across the hops are three too many)
      gin = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.gi0[(int64_t)step * a.gstride + b])));
      gfo = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.gf0[(int64_t)step * a.gstride + b])));
      gratio = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, gfo / fmaxf(gin, 1e-30f))));
    }
    const uint16_t* aux1 = (USERV && a.a1) ? (a.a1_last_only ? (step == a.nsteps - 1 ? a.a1 : nullptr) : a.a1 + (int64_t)step * a.a1stride) : nullptr;
    // Inline pack: the 128-node rounds of a step's input are laid out ONE HOP ahead of "during the step before": hop i of step t takes
    // round i + 1 of x_{t+1}, the step's last hop round 0 of x_{t+2}. x_{t+1} is then complete (stored, waited for, behind a barrier) when
    // step t's last epilogue requests it -- and recent: an input laid out a whole step earlier has left the caches by the time it is read
    // (the requests of all CUs then run at HBM latency: ~190 instead of ~70 units per step, profiles/r04_seq32_stamps_*). The caller lays
    // out steps 0 and 1.
    const bool pk_any = PKV && a.pk_src0 != nullptr;
    const int ubstride = a.ubstride;
    // (MODE 1: the pack lays out the operand of the NEXT item of this workgroup's loop, item nb = (t', b') = (nb / hmod, nb % hmod))
    const int nb = b + (int)gridDim.x;
    const int nbq = ITEMS ? __builtin_amdgcn_readfirstlane(nb / a.hmod) : 0, nbr = ITEMS ? __builtin_amdgcn_readfirstlane(nb - nbq * a.hmod) : 0;      // (scalar registers)
    const int64_t pk_soff = ITEMS ? (int64_t)nbr * a.pk_stride + (int64_t)nbq * a.pksrc_stride : (int64_t)b * a.pk_stride;
    const int pk_db = ITEMS ? nb : b;
    const __amdgpu_buffer_rsrc_t rsrc_o = __builtin_amdgcn_make_buffer_rsrc(hout, 0, hout ? B * (NP * F * 2) : 0, 0x00020000);
    [[maybe_unused]] const bool stamp_on = (step == (a.nsteps > 2 ? a.nsteps - 3 : 0)) && b == wg_seq;      // a typical step (diagnostic builds)
    GCRNN_STAMP32(0);
    const bool more = step + 1 < a.nsteps;      // the next step's operand is requested at the start of this step's last epilogue
    const __amdgpu_buffer_rsrc_t rsrc_xn = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(XS > 0 ? a.x0 + (int64_t)(step + 1) * a.xstride : nullptr), 0, (more && XS > 0) ? B * (NP * G * 2) : 0, 0x00020000);

    f32x4 acc[STILES][2];
    // acc[i][h] += W_tap(c, half h) [h|x]^T for the wave's 8 tiles: one weight fragment feeds 8 independent MFMA chains
    // (ch: the chunk the tap belongs to -- RT > 0: item (step NCH + ch) K + (K-1 - tap) of the order, in slot item % 3)
    auto tap_off = [&](int ch, int tap) -> uint32_t {
      if constexpr (RINGV) return ((uint32_t)((step * NCH + ch) * K + (K - 1 - tap)) % 3u) * (uint32_t)TAPB;
      else return (uint32_t)(tap * TAPB);
    };
    auto taps = [&](int ch, int tap, [[maybe_unused]] bool on_sums = false) {
#ifdef GCRNN_SEQ32_EXPERIMENT_NO_HOP_TAPS      // timing experiment, WRONG results: what would a hop cost if its tap were free (hidden inside the stream)?
      if (tap != K - 1) return;
#endif
      const int ln = lane_now();                       // (the fragment address is re-derived per call, not kept -- or spilled -- across the hops)
      const uint32_t wofs = (uint32_t)WOFF + (uint32_t)ln * 16u + tap_off(ch, tap);
      if constexpr (GATED) {
        // gi (x W_x) + gf (h W_h) on ONE accumulator chain per half: h-chain, scale by gf / gi, continue with x, scale by gi (gi = sigmoid(.) > 0;
        // the wave-uniform guard covers an underflowed gate). Waves 4..7 (tap first): the accumulators are ZERO on entry and the stream then
        // adds the hop's sums to the finished tap.
        // on_sums (the waves that stream first): the accumulators hold the hop's sums S; S + gf hW + gi xW comes out of the same chain started
        // from S / gf (three more roundings at 1e-7 relative; an underflowed forget gate skips the h-chain instead)
        const bool xpart = gin > 1e-30f;
        const bool hpart = !on_sums || gfo > 1e-30f;
        if (on_sums) {
          const float pre = hpart ? 1.f / gfo : (xpart ? 1.f / gin : 1.f);
#pragma unroll
          for (int i = 0; i < STILES; ++i) { acc[i][0] *= pre; acc[i][1] *= pre; }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (hpart) {
#pragma unroll
            for (int s = 0; s < HS; ++s) {
              const bf16x8 afr = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(smem + wofs + (uint32_t)((h * KS + s) * 1024)));
#pragma unroll
              for (int i = 0; i < STILES; ++i) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr[i][s], acc[i][h], 0, 0, 0);
            }
          }
          if (hpart) {
#pragma unroll
            for (int i = 0; i < STILES; ++i) acc[i][h] *= (xpart ? gratio : gfo);
          }
          if (xpart) {
#pragma unroll
            for (int s = HS; s < KS; ++s) {
              const bf16x8 afr = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(smem + wofs + (uint32_t)((h * KS + s) * 1024)));
#pragma unroll
              for (int i = 0; i < STILES; ++i) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr[i][s], acc[i][h], 0, 0, 0);
            }
            if constexpr (GATED) {
#pragma unroll
              for (int i = 0; i < STILES; ++i) acc[i][h] *= gin;
            }
          }
        }
      } else if constexpr (ITEMS) {
        // (gate pre-pass / filter-output pass; with an all-zero h0 the state half of the operand is neither loaded nor multiplied)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            if (s < HS && skip_h) continue;
            const bf16x8 afr = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(smem + wofs + (uint32_t)((h * KS + s) * 1024)));
#pragma unroll
            for (int i = 0; i < STILES; ++i) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr[i][s], acc[i][h], 0, 0, 0);
          }
      } else {
      // (the next fragment is requested before the current one's eight MFMAs)
      uint4 af[2];
      af[0] = *reinterpret_cast<const uint4*>(smem + wofs);
#pragma unroll
      for (int hs = 0; hs < 2 * KS; ++hs) {
        const int h = hs / KS, s = hs - h * KS;
        if (hs + 1 < 2 * KS) af[(hs + 1) & 1] = *reinterpret_cast<const uint4*>(smem + wofs + (uint32_t)((hs + 1) * 1024));
        const bf16x8 afr = __builtin_bit_cast(bf16x8, af[hs & 1]);
#pragma unroll
        for (int i = 0; i < STILES; ++i) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr[i][s], acc[i][h], 0, 0, 0);
      }
      }
    };
    // R1, tprime: the accumulators hold t / b (a wave that taps first carries the hop in t' = t / b -- see the hop): the image's a (.) t is (a b) (.) t'
    auto put = [&](auto tpc) __attribute__((always_inline)) {
      constexpr bool tprime = decltype(tpc)::value;
      int sw[STILES];
      slot_words(lane_now(), sw);
#pragma unroll
      for (int i = 0; i < STILES; ++i) {
        const int wv = sw[i];
        if constexpr (R1) {      // the image holds a (.) v
          const int slot = (wave * STILES + i) * 16 + (lane_now() & 15);
          float av = r1tab[slot];
          if constexpr (tprime) { const float bv = r1tab[NP + slot]; av *= (bv == 0.f ? 1.f : bv); }
          state_put<true>(reinterpret_cast<float*>(smem), wv, acc[i][0] * av);
          state_put<true>(reinterpret_cast<float*>(smem + PL), wv, acc[i][1] * av);
        } else {
          state_put<true>(reinterpret_cast<float*>(smem), wv, acc[i][0]);
          state_put<true>(reinterpret_cast<float*>(smem + PL), wv, acc[i][1]);
        }
      }
    };
    // seed of a chunk: tap K-1 goes straight into the hop image (every wave has left the image: the barrier before)
    auto seed = [&](int ch) {
#pragma unroll
      for (int i = 0; i < STILES; ++i) { acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      taps(ch, K - 1);
      put(std::false_type{});
    };
    // The seed's tap alone, for the chunk boundaries where it runs beside the user-layout row stores: it reads the operand and the weight
    // fragments only, so the image's place may still hold the transposed tile.
    auto seed_taps_beside_rows = [&](int ch) {
#pragma unroll
      for (int i = 0; i < STILES; ++i) { acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      taps(ch, K - 1);
    };
    seed(chunk0);

#pragma unroll 1
    for (int chunk = chunk0; chunk < (SPLIT ? chunk0 + 1 : NCH); ++chunk) {
      // opaque per chunk: index arithmetic is re-derived from it inside the loop -- hoisted out it would have to be spilled
      // (nothing derived from the lane id lives across the hops: every use below re-derives it, lane_now())
      const bool last = SPLIT || chunk == NCH - 1;
      lds_barrier();      // the seed is in the image
      GCRNN_STAMP32(1 + chunk * 24);

      // virtual round v of this step (NRND per step, shifted by one hop) -> (target step, round); false: nothing to lay out
      auto pack_target = [&](int v, int& tgt, int& rnd) -> bool {
        if constexpr (ITEMS) {      // the workgroup's next item, round v (its operand is read when that item starts)
          rnd = v; tgt = 0;
          return pk_any && v < NRND && nb < B;
        }
        if constexpr (SPLIT) {      // one step per launch: this workgroup's rounds (those of its chunk's hops) of the NEXT step's input, the host has set the pointers
          rnd = v; tgt = 0;
          return pk_any && v < NRND;
        }
        if constexpr (MODE == 2) {      // step i lays out the upstream gradient step i + 1's epilogue reads (the caller laid out step 0's)
          rnd = v; tgt = step + 1;
          return pk_any && v < NRND && tgt < a.nsteps - (a.final_raw ? 1 : 0);
        }
        v += RPH;
        const int wrap = v >= NRND ? 1 : 0;
        rnd = v - wrap * NRND;
        tgt = step + 1 + wrap;
        return pk_any && tgt >= (self_start ? 1 : 2) && tgt < a.nsteps;      // (self-start: step 0's rounds lay out x_1 too -- rounds >= RPH of it)
      };
      // inline pack, round rnd of step tgt: x_tgt[:, rnd * 128 .. + 127] (user layout, rows = features) by LDS-DMA into the tile ...
      auto pack_issue = [&](int v) {
        int tgt, rnd;
        if (!pack_target(v, tgt, rnd)) return;
        const uint16_t* pk_src = a.pk_src0 + ((ITEMS || SPLIT) ? 0 : (int64_t)tgt * a.pksrc_stride);
        constexpr int PPR = NPCK / 8, PIECES = PKROWS * PPR;
        static_assert(PIECES % STHREADS == 0, "whole pieces per thread");
        const uint16_t* xsrc = pk_src + pk_soff + rnd * NPCK;
        const int tl = wave * 64 + lane_now();
#pragma unroll
        for (int i = 0; i < PIECES / STHREADS; ++i) {
          const int id = i * STHREADS + tl;
          const int row = id / PPR, cs = id - row * PPR;
          const int col = (cs - (row >> 3)) & (PPR - 1);
          if (rnd * NPCK + col * 8 < N)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xsrc + (int64_t)row * N + col * 8),
                                             (__attribute__((address_space(3))) void*)(xtile + (i * STHREADS + wave * 64) * 16), 16, 0, GCRNN_SEQ32_NT_DMA);
        }
      };
      // ... and out of it transposed: whole sequence-major rows [node][features]
      auto pack_drain = [&](int v) {
        int tgt, rnd;
        if (!pack_target(v, tgt, rnd)) return;
        uint16_t* pk_dst = a.pk_dst0 + ((ITEMS || SPLIT) ? 0 : (int64_t)tgt * a.pkdst_stride);
        constexpr int PCS = PKROWS / 8, RI = PCS * NPCK / STHREADS;
        static_assert(PCS * NPCK % STHREADS == 0, "whole row pieces per thread");
        typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int u32x4_t;
        const __amdgpu_buffer_rsrc_t rsrc_pk = __builtin_amdgcn_make_buffer_rsrc(pk_dst, 0, B * (NP * PKROWS * 2), 0x00020000);
        const int tl = wave * 64 + lane_now();
        u32x4_t vv[RI];
        // the tile's 2-byte columns of this thread's row piece(s): ALL reads in flight, one wait (hipcc waits after every pair: eight LDS round
        // trips per piece, ~8 of a hop's ~19 units of write-back; d16 loads cannot merge the halves -- with SRAM-ECC they rewrite the whole register)
        static_assert(RI == 1 || RI == 2, "one or two row pieces per thread");
        uint32_t h16[RI][8];
        uint32_t sa[RI];
#pragma unroll
        for (int i = 0; i < RI; ++i) {
          const int id = i * STHREADS + tl;
          const int nl = id / PCS, pc = id - nl * PCS;
          sa[i] = (uint32_t)(xtile - smem) + (uint32_t)((pc * 8) * (NPCK * 2) + ((nl + 8 * pc) & (NPCK - 1)) * 2);
        }
        static_assert(NPCK * 2 == 256, "row pitch of the pack tile in the asm offsets");
        if constexpr (RI == 2) {
          asm volatile("ds_read_u16 %0, %16\n\tds_read_u16 %1, %16 offset:256\n\tds_read_u16 %2, %16 offset:512\n\tds_read_u16 %3, %16 offset:768\n\t"
                       "ds_read_u16 %4, %16 offset:1024\n\tds_read_u16 %5, %16 offset:1280\n\tds_read_u16 %6, %16 offset:1536\n\tds_read_u16 %7, %16 offset:1792\n\t"
                       "ds_read_u16 %8, %17\n\tds_read_u16 %9, %17 offset:256\n\tds_read_u16 %10, %17 offset:512\n\tds_read_u16 %11, %17 offset:768\n\t"
                       "ds_read_u16 %12, %17 offset:1024\n\tds_read_u16 %13, %17 offset:1280\n\tds_read_u16 %14, %17 offset:1536\n\tds_read_u16 %15, %17 offset:1792\n\t"
                       "s_waitcnt lgkmcnt(0)"
                       : "=&v"(h16[0][0]), "=&v"(h16[0][1]), "=&v"(h16[0][2]), "=&v"(h16[0][3]), "=&v"(h16[0][4]), "=&v"(h16[0][5]), "=&v"(h16[0][6]), "=&v"(h16[0][7]),
                         "=&v"(h16[RI - 1][0]), "=&v"(h16[RI - 1][1]), "=&v"(h16[RI - 1][2]), "=&v"(h16[RI - 1][3]), "=&v"(h16[RI - 1][4]), "=&v"(h16[RI - 1][5]), "=&v"(h16[RI - 1][6]), "=&v"(h16[RI - 1][7])
                       : "v"(sa[0]), "v"(sa[RI - 1]));
        } else {
          asm volatile("ds_read_u16 %0, %8\n\tds_read_u16 %1, %8 offset:256\n\tds_read_u16 %2, %8 offset:512\n\tds_read_u16 %3, %8 offset:768\n\t"
                       "ds_read_u16 %4, %8 offset:1024\n\tds_read_u16 %5, %8 offset:1280\n\tds_read_u16 %6, %8 offset:1536\n\tds_read_u16 %7, %8 offset:1792\n\t"
                       "s_waitcnt lgkmcnt(0)"
                       : "=&v"(h16[0][0]), "=&v"(h16[0][1]), "=&v"(h16[0][2]), "=&v"(h16[0][3]), "=&v"(h16[0][4]), "=&v"(h16[0][5]), "=&v"(h16[0][6]), "=&v"(h16[0][7])
                       : "v"(sa[0]));
        }
#pragma unroll
        for (int i = 0; i < RI; ++i) {
          const int id = i * STHREADS + tl;
          const int nl = id / PCS;
          const bool ok = rnd * NPCK + nl < N;
          uint32_t w4[4];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) w4[jj] = h16[i][2 * jj] | (h16[i][2 * jj + 1] << 16);
          vv[i] = u32x4_t{ok ? w4[0] : 0u, ok ? w4[1] : 0u, ok ? w4[2] : 0u, ok ? w4[3] : 0u};
        }
#pragma unroll
        for (int i = 0; i < RI; ++i) asm volatile("" : "+v"(vv[i]));          // every piece in its own tuple before the first store (gfx950 store-data hazard)
#pragma unroll
        for (int i = 0; i < RI; ++i) {
          const int id = i * STHREADS + tl;
          const int nl = id / PCS, pc = id - nl * PCS;
          __builtin_amdgcn_raw_buffer_store_b128(vv[i], rsrc_pk, (rnd * NPCK + nl) * (PKROWS * 2) + pc * 16 + pk_db * (NP * PKROWS * 2), 0, 0);
        }
      };

      // Weight fragments of chunk wc, tap `tap` -> their place in LDS (2 KS pieces of 1 KB). One tap at a time, into a place whose last
      // reader is a barrier behind: during hop j the NEXT chunk's tap K - j (read by this chunk's seed / hop j - 1), during hop 1 also this
      // chunk's own tap 0 (its place still held the previous chunk's, read at that chunk's last hop). Every piece is covered by the hop's
      // vmcnt(0) + barrier, and no LDS-DMA is pending during an epilogue -- hipcc orders each LDS access of a wave behind its pending
      // LDS-DMA pieces with a vmcnt(0), which in the last epilogue would also wait for the next operand's requests.
      auto r0_of = [&](int j) { return (chunk * (K - 1) + (j - 1)) * RPH; };
      // RT > 0 (the ring): hop j reads item j of its chunk (the seed item 0) and brings item j + 2 -- hop 1 also item 2 -- into the slots of
      // items j - 1 (read in hop j - 1, or by the seed in front of the chunk's first barrier) and -1 (the previous chunk's tap 0, read in its
      // last hop): K items in K - 1 hops as before, in front of the stream as before, each covered by its hop's wait, two hops ahead of its
      // reader instead of a chunk ahead. Items K and K + 1 are the next chunk's taps K-1 and K-2: both have landed when the seed taps run
      // beside the row stores, and no LDS-DMA is pending in an epilogue -- at K = 2 either, which needs no wait at the chunk's end any more.
      auto weights_issue = [&](int wc, int tap, uint32_t dst = 0xffffffffu) {
        if (dst == 0xffffffffu) dst = (uint32_t)(tap * TAPB);
        const char* wsrc = reinterpret_cast<const char*>(a.wpack) + (size_t)wc * WCH + (size_t)tap * (2 * KS * 1024);
        const int lane = lane_now();
#pragma unroll
        for (int i = 0; i < (2 * KS + SWAVES - 1) / SWAVES; ++i) {
          const int piece = i * SWAVES + wave;
          if (piece < 2 * KS)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc + piece * 1024 + lane * 16),
                                             (__attribute__((address_space(3))) void*)(smem + WOFF + dst + piece * 1024), 16, 0, 0);
        }
      };
      [[maybe_unused]] auto ring_issue = [&](int pos) {      // item `pos` of this chunk's order, K <= pos: the next chunk's
        const int nx = pos >= K ? 1 : 0;
        weights_issue(nx ? (chunk + 1) % NCH : chunk, K - 1 - (pos - nx * K), ((uint32_t)((step * NCH + chunk) * K + pos) % 3u) * (uint32_t)TAPB);
      };
      // MODE 2: the epilogue's operands h_{t-1}, dH_{t-1} of this lane's (node, 8 features) per tile. Requested in the write-back phases of hops
      // 1 .. EPH (behind the hop's vmcnt(0) + barrier), a share of the tiles each: they land under the NEXT hop's stream and are covered by its
      // vmcnt(0). Requested in front of hop 1 (round 4's first form; still so for K < 4) the waves that tap first met hipcc's vmcnt(0) in front
      // of the tap's weight reads a few hundred cycles later and sat out the whole HBM latency: hop 1 took ~200 units instead of ~75
      // (profiles/r04_seq32_stamps_chain.txt).
      typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int u32x4e_t;
      [[maybe_unused]] u32x4e_t eph[MODE == 2 ? STILES : 1], epg[(SONLY && !UPR1) ? STILES : 1];
      [[maybe_unused]] uint32_t epy[UPR1 ? STILES : 1];      // UPR1: dy_{t-1} of this lane's node per tile (bf16 bits)
      [[maybe_unused]] float epn[MODE == 4 ? STILES : 1][2];      // MODE 4: this lane's node's input / forget gate per tile
#ifndef GCRNN_SEQ32_EP_FIRST
#define GCRNN_SEQ32_EP_FIRST 1      // the requests in front of the hop's write-back (0: behind it; same-box A/B: profiles/r04_seq32_chain_requests_ab.txt)
#endif
#ifndef GCRNN_SEQ32_EP_EARLY
#define GCRNN_SEQ32_EP_EARLY 0      // 1: all of them in front of hop 1 (A/B)
#endif
      constexpr int EPH = (SONLY && K >= 4 && !GCRNN_SEQ32_EP_EARLY) ? K - 2 : 0;
      auto ep_request = [&](auto i0c, auto i1c) __attribute__((always_inline)) {
        if constexpr (MODE == 4) {
          constexpr int I0 = decltype(i0c)::value, I1 = decltype(i1c)::value;
          const int lq = lane_now();
          int swp[STILES];
          slot_words(lq, swp);
          const __amdgpu_buffer_rsrc_t rsrc_eg = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(ep_dh), 0, ep_dh ? B * (NP * F * 2) : 0, 0x00020000);
          const __amdgpu_buffer_rsrc_t rsrc_n = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ep_ng), 0, (int)(a.nghalf * 8), 0x00020000);      // ni | nf, 2 x nghalf floats; rows >= N: out of range -> 0
#pragma unroll
          for (int i = I0; i < I1; ++i) {
            const int node = swp[i] >> 16;
            epg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_eg, node * (F * 2) + (chunk * 32 + (lq >> 4) * 8) * 2, b * (NP * F * 2), 0);
            const int go = node < N ? (b * N + node) * 4 : 0x7ffffff0;
            epn[i][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_n, go, 0, 0));
            epn[i][1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_n, go, (int)(a.nghalf * 4), 0));
          }
        }
        if constexpr (MODE == 2) {
          constexpr int I0 = decltype(i0c)::value, I1 = decltype(i1c)::value;
          const int lq = lane_now();
          int swp[STILES];
          slot_words(lq, swp);
          const __amdgpu_buffer_rsrc_t rsrc_eh = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(ep_h), 0, ep_h ? B * (NP * F * 2) : 0, 0x00020000);
          // (UPR1: the row dy[b][t-1][0 .. N) alone -- padding slots carry nodes >= N, out of range: they read 0)
          const __amdgpu_buffer_rsrc_t rsrc_eg = UPR1 ? __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(ep_dy), 0, ep_dy ? N * 2 : 0, 0x00020000)
                                                      : __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(ep_dh), 0, ep_dh ? B * (NP * F * 2) : 0, 0x00020000);
#pragma unroll
          for (int i = I0; i < I1; ++i) {
            const int eoff = (swp[i] >> 16) * (F * 2) + (chunk * 32 + (lq >> 4) * 8) * 2;
            eph[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_eh, eoff, b * (NP * F * 2), 0);
            if constexpr (UPR1) epy[i] = __builtin_amdgcn_raw_buffer_load_b16(rsrc_eg, (swp[i] >> 16) * 2, 0, 0);
            else epg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_eg, eoff, b * (NP * F * 2), 0);
          }
        }
      };
      if constexpr (SONLY && EPH == 0) ep_request(std::integral_constant<int, 0>{}, std::integral_constant<int, STILES>{});
      // ---- Horner hops on the two-plane bf16 image; the tap a hop adds accumulates onto its sums --------------------------------
      auto hop = [&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        auto dma_issue = [&]() {      // this wave's LDS-DMA pieces of the hop, right in front of its stream
          if constexpr (RINGV) {
            if (j == 1) ring_issue(2);
            ring_issue(j + 2);
          } else
          if (NCH > 1 && !SPLIT) {
            weights_issue((chunk + 1) % NCH, K - j);
            if (j == 1 && K > 2) weights_issue(chunk, 0);
          }
          if (r0_of(j) < NRND) pack_issue(r0_of(j));
        };
        const int r0 = r0_of(j);      // this hop's first pack round
        // The two waves of a SIMD take the hop's two phases in opposite order: issue arbitration favours the older wave, so with all
        // eight streaming at once waves 4..7 finish their streams ~30 % after waves 0..3 and only then start their tap MFMAs while the
        // others wait at the barrier (profiles/r04_seq32_stamps_native_same_order.txt). The tap of a hop does not depend on its sums
        // (D = A B + D accumulates either way), so waves 4..7 evaluate it FIRST: their MFMAs run beside the streams of waves 0..3, which
        // then have the LDS to four waves, and the other way round afterwards.
#pragma unroll
        for (int i = 0; i < STILES; ++i) { acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        // (the pack's LDS-DMA pieces go out right before the wave's stream: hipcc orders every later LDS read of the wave behind them with a
        //  vmcnt(0) -- behind the stream that wait is free, in front of the tap's weight reads it would expose the pieces' whole latency)
        // R1 (S = a b^T on its pattern): a hop is t_j = u_j + b (.) sum (a (.) t_{j+1}). A wave that streams first scales its sums by b and adds the
        // tap (it carries t; image write: a (.) t). A wave that taps first cannot scale the sums alone once the tap is in the accumulator -- it
        // carries t' = t / b instead: t'_j = u_j / b + sum, image write (a b) (.) t', and b (.) t' after the chunk's last hop (b = 0: no
        // in-neighbours, the sum is empty: factor 1). All in fp32 registers; round 4's first R1 made every wave stream first (-13 %).
        const bool stream_first = (!GATED || !GCRNN_SEQ32_GATED_TAPS_FIRST) && (wave < SWAVES / 2 || GCRNN_SEQ32_SAME_ORDER || (R1 && GCRNN_SEQ32_R1_STREAM_FIRST));
        if (stream_first) {
          dma_issue();
          GCRNN_HOP_ASM_WIDE32_STREAM(acc);
          r1_scale(acc, 0);      // R1: sums of a (.) v over the in-neighbours, times b[n]: then the tap
          GCRNN_STAMP32(1 + chunk * 24 + 4 * (j - 1) + 1);
          if (j == 2 && chunk == 0) GCRNN_STAMP32_WAVE(56);
          taps(chunk, K - 1 - j, true);
        } else {
          taps(chunk, K - 1 - j);
          r1_scale(acc, 1);      // R1: the tap in units of b (t' = t / b)
          if (j == 2 && chunk == 0) GCRNN_STAMP32_WAVE(56);
          dma_issue();
#if GCRNN_SEQ32_YOUNG_PRIO      // experiment: the younger wave of each SIMD streams at raised issue priority (it starts its stream a tap later)
          __builtin_amdgcn_s_setprio(GCRNN_SEQ32_YOUNG_PRIO);
#endif
          GCRNN_HOP_ASM_WIDE32_STREAM(acc);
#if GCRNN_SEQ32_YOUNG_PRIO
          __builtin_amdgcn_s_setprio(0);
#endif
        }
        GCRNN_STAMP32(1 + chunk * 24 + 4 * (j - 1) + 2);
        if (j == 2 && chunk == 0) GCRNN_STAMP32_WAVE(64);
        if (pk_any || (NCH > 1 && !SPLIT)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's LDS-DMA pieces have landed (they had the stream)
        lds_barrier();      // every wave has left the image (and the weights, after the last hop); every piece of the pack tile is in
        GCRNN_STAMP32(1 + chunk * 24 + 4 * (j - 1) + 3);
#if GCRNN_SEQ32_EP_FIRST      // (A/B: the requests in front of the write-back instead of behind it)
        if constexpr (SONLY && EPH > 0 && j <= EPH)
          ep_request(std::integral_constant<int, (j - 1) * STILES / (EPH > 0 ? EPH : 1)>{}, std::integral_constant<int, j * STILES / (EPH > 0 ? EPH : 1)>{});
#endif
        if (j < K - 1) {
          if (R1 && !stream_first) put(std::true_type{});
          else put(std::false_type{});
        }
        if constexpr (R1 && j == K - 1) {
          if (!stream_first) r1_scale(acc, 2);      // the chunk's result: t_0 = b (.) t'_0
        }
        if (K == 2 && NCH > 1 && !SPLIT && !RINGV) weights_issue((chunk + 1) % NCH, 0);      // (K = 2: tap 0's fragments are free only now, and needed at the next chunk's only hop)
        if (r0 < NRND) pack_drain(r0);
#pragma unroll
        for (int e = 1; e < RPH; ++e) {       // (fewer hops than rounds: the extra rounds are not hidden behind a stream)
          if (pk_any && r0 + e < NRND) {
            lds_barrier();
            pack_issue(r0 + e);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            lds_barrier();
            pack_drain(r0 + e);
          }
        }
#if !GCRNN_SEQ32_EP_FIRST
        if constexpr (SONLY && EPH > 0 && j <= EPH)
          ep_request(std::integral_constant<int, (j - 1) * STILES / (EPH > 0 ? EPH : 1)>{}, std::integral_constant<int, j * STILES / (EPH > 0 ? EPH : 1)>{});
#endif
        if (j < K - 1) lds_barrier();      // the image is complete (and the pack tile read)
        GCRNN_STAMP32(1 + chunk * 24 + 4 * (j - 1) + 4);
      };
      seq_static_for(hop, std::make_integer_sequence<int, K - 1>{});

      // ---- epilogue: + 2 b, tanh, bf16; lane (r, q) holds features 32 c + 8 q .. + 7 of its node: ONE 16-byte store per tile ------------
      typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int u32x4_t;
      const int lane = lane_now(), q = lane >> 4;
      // VAR bit 2: this workgroup's state scratch (scalar registers, made where it is used)
      auto scratch_rsrc = [&]() {
        return __builtin_amdgcn_make_buffer_rsrc(SCRV ? a.scr + (int64_t)blockIdx.x * ((HS - 1) * (SCR_CH / 2)) : nullptr, 0, SCRV ? (HS - 1) * SCR_CH : 0, 0x00020000);
      };
      auto request_next_operand = [&]() {
        if (ITEMS || !(last && more)) return;
        // the next step's operand: x_{t+1} (laid out two steps ahead, or by the caller) and the state features of the earlier chunks
        // (stored -- and waited for -- at their chunk's end); the last chunk's come from this epilogue's registers below
        const int qo = lane_now() >> 4;
        int sw[STILES];
        slot_words(lane, sw);
        const __amdgpu_buffer_rsrc_t rsrc_hn = __builtin_amdgcn_make_buffer_rsrc(SCRV ? nullptr : hout, 0, SCRV ? 0 : B * (NP * F * 2), 0x00020000);
        [[maybe_unused]] const __amdgpu_buffer_rsrc_t rsrc_sn = scratch_rsrc();
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          if (s == HS - 1) continue;
#pragma unroll
          for (int i = 0; i < STILES; ++i) {
            const int w = sw[i];
#ifdef GCRNN_SEQ32_EXPERIMENT_SKIP      // timing experiment, WRONG results: 1 = no state requests, 2 = no input requests (which half of the operand costs the wait?)
            if ((GCRNN_SEQ32_EXPERIMENT_SKIP == 1) == (s < HS)) continue;
#endif
            if (RINGV && s < HS && i < RT)      // resident tile: this lane's own 16 bytes of the wave's block (no barrier: the wave wrote them itself, in chunk s's epilogue)
              bfr[i][s] = *reinterpret_cast<const bf16x8*>(smem + M::RES_OFF + ((s * SWAVES + wave) * RT + i) * 1024 + lane_now() * 16);
            else if (SCRV && s < HS)      // this lane's own 16 bytes of the scratch (slot order: no slot word), sc1
              bfr[i][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_sn, (lane_now() & 15) * 64 + 16 * qo, s * SCR_CH + (wave * STILES + i) * 1024, 16));
            else if (s < HS)
              bfr[i][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_hn, (w >> 16) * (F * 2) + 16 * qo + 64 * s, b * (NP * F * 2), GCRNN_SEQ32_NT_XLOAD));
            else
              bfr[i][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_xn, (w >> 16) * (G * 2) + 16 * qo + 64 * (s - HS), b * (NP * G * 2), GCRNN_SEQ32_NT_XLOAD));
          }
        }
      };
      if (GCRNN_SEQ32_OPERAND_AT == 0) request_next_operand();
      if (ITEMS) GCRNN_STAMP32(1 + chunk * 24 + 19);      // (diagnostic builds: start of the epilogue proper)
      float bs[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) bs[h][e] = (MODE >= 3 ? 1.f : (gin + gfo)) * lbias[chunk * 32 + q * 8 + h * 4 + e];      // (modes 3, 4: ONE filter's bias)      // the one bias is added by both filters (graphML.py:2420-2421): 2 b, or (gi + gf) b
      u32x4_t pkd[STILES];
      int swe[STILES];
      slot_words(lane, swe);
      if constexpr (MODE == 1) {
        // gate pre-pass: c = tanh(pre) of this gate's sub-cell (chunk / HS = the gate), partial dot product with its read-out weights
        // [N][F] fp32 (graphML.py:2364-2366: vec over (f, n)), one partial per (chunk, wave) -- the caller adds them in a fixed order; with
        // output arrays the sub-cell's state is stored (bf16) for the gate's BPTT. The weights are shared by every item (L2-resident); two
        // tiles' worth are requested at a time.
        const int gate = chunk / HS, cg = chunk - gate * HS;
        if (a.tapf) {
          // node gates: s_k[n] += sum_f c[n][f] w_k[f] over this chunk's 32 features on the matrix cores -- the lane's packed state (node r, features
          // 8 q .. + 7) IS the B fragment (k = feature, n = node), the taps' three bf16 planes the A fragments (m = tap): rows 4 q' + e of D are
          // taps, columns nodes; the chunk's partial goes to memory (the two chunks of a gate are added by the caller, fixed order)
          typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int u32x4t;
          const uint4* tfp = a.tapf + ((size_t)(gate * HS + cg) * 3) * 64 + lane;
          bf16x8 ta[3];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) ta[pl] = __builtin_bit_cast(bf16x8, tfp[pl * 64]);
          const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(gate ? a.out1 : a.out0, 0, (gate ? a.out1 : a.out0) ? B * (NP * F * 2) : 0, 0x00020000);
          float* so = a.taps_out + (((int64_t)b * 2 + gate) * HS + cg) * (int64_t)a.ntaps * N;
#pragma unroll
          for (int i = 0; i < STILES; ++i) {
            const int node = swe[i] >> 16;
            u32x4t p{0u, 0u, 0u, 0u};
            if (node < N) {
              const f32x4 a0 = acc[i][0], a1 = acc[i][1];
              p[0] = pack2bf(fast_tanh(a0[0] + bs[0][0]), fast_tanh(a0[1] + bs[0][1]));
              p[1] = pack2bf(fast_tanh(a0[2] + bs[0][2]), fast_tanh(a0[3] + bs[0][3]));
              p[2] = pack2bf(fast_tanh(a1[0] + bs[1][0]), fast_tanh(a1[1] + bs[1][1]));
              p[3] = pack2bf(fast_tanh(a1[2] + bs[1][2]), fast_tanh(a1[3] + bs[1][3]));
            }
            if (gate ? a.out1 : a.out0) __builtin_amdgcn_raw_buffer_store_b128(p, rsrc_c, node * (F * 2) + (cg * 32 + q * 8) * 2, b * (NP * F * 2), 0);
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int pl = 2; pl >= 0; --pl) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ta[pl], __builtin_bit_cast(bf16x8, p), d, 0, 0, 0);
            // D rows 4 q + e = taps, column r = this lane's node of the tile
            if (node < N) {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (q * 4 + e < a.ntaps) so[(int64_t)(q * 4 + e) * N + node] = d[e];
            }
          }
        } else {
        const float* gwp = a.gw + (int64_t)gate * N * F + cg * 32 + q * 8;
        uint16_t* cso = gate ? a.out1 : a.out0;
        const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(cso, 0, cso ? B * (NP * F * 2) : 0, 0x00020000);
        float part = 0.f;
        // (the read-out weights of the NEXT two tiles are requested before this pair is evaluated: one L2 round trip per chunk is exposed instead
        //  of four; -0.6 % on the time-gated forward, profiles/r04_seq32_gate_readout_ab.txt. The same weights as bf16 -- half the bytes -- ran
        //  SLOWER: this epilogue, 95 units per chunk against the recurrence's 35 in r04_seq32_stamps_gate_pair.txt, is not bound by their bytes)
#ifndef GCRNN_SEQ32_GATE_W_PIPELINE
#define GCRNN_SEQ32_GATE_W_PIPELINE 1
#endif
        float4 w8s[2][2][2];
        auto w8_load = [&](int set, int i0l) __attribute__((always_inline)) {
#pragma unroll
          for (int t2 = 0; t2 < 2; ++t2) {
            const int nd = (swe[i0l + t2] >> 16) < N ? (swe[i0l + t2] >> 16) : N - 1;
            w8s[set][t2][0] = *reinterpret_cast<const float4*>(gwp + (int64_t)nd * F);
            w8s[set][t2][1] = *reinterpret_cast<const float4*>(gwp + (int64_t)nd * F + 4);
          }
        };
        if (GCRNN_SEQ32_GATE_W_PIPELINE) w8_load(0, 0);
#pragma unroll
        for (int i0 = 0; i0 < STILES; i0 += 2) {
          const int wset = GCRNN_SEQ32_GATE_W_PIPELINE ? (i0 >> 1) & 1 : 0;
          if (GCRNN_SEQ32_GATE_W_PIPELINE) { if (i0 + 2 < STILES) w8_load(wset ^ 1, i0 + 2); }
          else w8_load(0, i0);
          const auto& w8 = w8s[wset];
#pragma unroll
          for (int t2 = 0; t2 < 2; ++t2) {
            const int i = i0 + t2;
            const int node = swe[i] >> 16;
            u32x4_t p{0u, 0u, 0u, 0u};
            if (node < N) {
              const f32x4 a0 = acc[i][0], a1 = acc[i][1];
              const float o0 = fast_tanh(a0[0] + bs[0][0]), o1 = fast_tanh(a0[1] + bs[0][1]), o2 = fast_tanh(a0[2] + bs[0][2]), o3 = fast_tanh(a0[3] + bs[0][3]);
              const float o4 = fast_tanh(a1[0] + bs[1][0]), o5 = fast_tanh(a1[1] + bs[1][1]), o6 = fast_tanh(a1[2] + bs[1][2]), o7 = fast_tanh(a1[3] + bs[1][3]);
              // (explicit chain: with -ffp-contract=fast the association of a*b + c*d + .. would be the compiler's choice per instantiation)
              part = __builtin_fmaf(o3, w8[t2][0].w, __builtin_fmaf(o2, w8[t2][0].z, __builtin_fmaf(o1, w8[t2][0].y, __builtin_fmaf(o0, w8[t2][0].x, part))));
              part = __builtin_fmaf(o7, w8[t2][1].w, __builtin_fmaf(o6, w8[t2][1].z, __builtin_fmaf(o5, w8[t2][1].y, __builtin_fmaf(o4, w8[t2][1].x, part))));
              p[0] = pack2bf(o0, o1); p[1] = pack2bf(o2, o3); p[2] = pack2bf(o4, o5); p[3] = pack2bf(o6, o7);
            }
            if (cso) __builtin_amdgcn_raw_buffer_store_b128(p, rsrc_c, node * (F * 2) + (cg * 32 + q * 8) * 2, b * (NP * F * 2), 0);
          }
        }
        GCRNN_STAMP32(1 + chunk * 24 + 18);      // (diagnostic builds: end of the tile loop)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
        if (lane == 0) a.go[(int64_t)b * (NCH * SWAVES) + chunk * SWAVES + wave] = part;
        }
      } else if constexpr (MODE == 3) {
        // filter-output pass: A(S) x_t + b as it is (bf16), [items][NP][F]
        const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(a.out0, 0, B * (NP * F * 2), 0x00020000);
#pragma unroll
        for (int i = 0; i < STILES; ++i) {
          const int node = swe[i] >> 16;
          u32x4_t p{0u, 0u, 0u, 0u};
          if (node < N) {
            const f32x4 a0 = acc[i][0], a1 = acc[i][1];
            p[0] = pack2bf(a0[0] + bs[0][0], a0[1] + bs[0][1]); p[1] = pack2bf(a0[2] + bs[0][2], a0[3] + bs[0][3]);
            p[2] = pack2bf(a1[0] + bs[1][0], a1[1] + bs[1][1]); p[3] = pack2bf(a1[2] + bs[1][2], a1[3] + bs[1][3]);
          }
          __builtin_amdgcn_raw_buffer_store_b128(p, rsrc_c, node * (F * 2) + (chunk * 32 + q * 8) * 2, b * (NP * F * 2), 0);
        }
      } else if constexpr (MODE == 4) {
        // node-gated step: the x part comes from the all-items pass, both parts are scaled per node (and per sequence)
#pragma unroll
        for (int i = 0; i < STILES; ++i) {
          const int node = swe[i] >> 16;
          u32x4_t p{0u, 0u, 0u, 0u};
          if (node < N) {
            const float ni = gin * epn[i][0], nf = gfo * epn[i][1];
            float yv[8], rw[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              yv[2 * e] = bf2f((uint16_t)(epg[i][e] & 0xffffu)); yv[2 * e + 1] = bf2f((uint16_t)(epg[i][e] >> 16));
              rw[e] = acc[i][0][e] + bs[0][e]; rw[4 + e] = acc[i][1][e] + bs[1][e];
            }
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = fast_tanh(ni * yv[e] + nf * rw[e]);
            p[0] = pack2bf(o[0], o[1]); p[1] = pack2bf(o[2], o[3]); p[2] = pack2bf(o[4], o[5]); p[3] = pack2bf(o[6], o[7]);
          }
          pkd[i] = p;
          __builtin_amdgcn_raw_buffer_store_b128(p, rsrc_o, node * (F * 2) + (chunk * 32 + q * 8) * 2, b * (NP * F * 2), 0);
        }
      } else if constexpr (MODE == 2) {
        // BPTT data step: the hops applied sum_k (S)^k (dpre_t B_k^T) = d h_{t-1} (recurrent part, scaled by the forget gate of the step it came
        // through); add the upstream gradient and go through tanh': dpre_{t-1} = (gsc acc + dH_{t-1}) (1 - h_{t-1}^2); without dH the raw state
        // gradient is stored (d h0). gpart: <h_{t-1}, acc> = <B(S) h_{t-1}, dpre_t> by the adjoint identity (the forget gate's gradient).
        float part = 0.f;
        [[maybe_unused]] float hw8[8];      // UPR1: the head's weights of this lane's eight features (for the epilogue only)
        if constexpr (UPR1) {
#pragma unroll
          for (int e = 0; e < 8; ++e) hw8[e] = lbias[chunk * 32 + q * 8 + e];
        }
#pragma unroll
        for (int i = 0; i < STILES; ++i) {
          const int node = swe[i] >> 16;
          float hv[8], gv[8], rw[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            hv[2 * e] = bf2f((uint16_t)(eph[i][e] & 0xffffu)); hv[2 * e + 1] = bf2f((uint16_t)(eph[i][e] >> 16));
            if constexpr (!UPR1) { gv[2 * e] = bf2f((uint16_t)(epg[i][e] & 0xffffu)); gv[2 * e + 1] = bf2f((uint16_t)(epg[i][e] >> 16)); }
            rw[e] = acc[i][0][e]; rw[4 + e] = acc[i][1][e];
          }
          if constexpr (UPR1) {      // dH = bf16(w dy), the fp32 product rounded to nearest-even: what the head's backward kernel stores
            const float dyv = bf2f((uint16_t)epy[i]);
#pragma unroll
            for (int e = 0; e < 8; ++e) gv[e] = bf2f(f2bf(hw8[e] * dyv));
          }
          if (gpart) {
#pragma unroll
            for (int e = 0; e < 8; ++e) part = __builtin_fmaf(rw[e], hv[e], part);      // (explicit chain; rows >= N of h are zero)
          }
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            o[e] = rw[e] * gsc;
            if (ep_up) o[e] = (o[e] + gv[e]) * (1.f - hv[e] * hv[e]);
          }
          u32x4_t p{0u, 0u, 0u, 0u};
          if (node < N) { p[0] = pack2bf(o[0], o[1]); p[1] = pack2bf(o[2], o[3]); p[2] = pack2bf(o[4], o[5]); p[3] = pack2bf(o[6], o[7]); }
          pkd[i] = p;
          __builtin_amdgcn_raw_buffer_store_b128(p, rsrc_o, node * (F * 2) + (chunk * 32 + q * 8) * 2, b * (NP * F * 2), 0);      // (dropped when there is no output array)
        }
        if (gpart) {
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
          if (lane == 0) gpart[(int64_t)b * (NCH * SWAVES) + chunk * SWAVES + wave] = part;
        }
      } else {
#pragma unroll
      for (int i = 0; i < STILES; ++i) {
        const int node = swe[i] >> 16;
        u32x4_t p{0u, 0u, 0u, 0u};
        if (node < N) {
          const f32x4 a0 = acc[i][0], a1 = acc[i][1];
          p[0] = pack2bf(fast_tanh(a0[0] + bs[0][0]), fast_tanh(a0[1] + bs[0][1]));
          p[1] = pack2bf(fast_tanh(a0[2] + bs[0][2]), fast_tanh(a0[3] + bs[0][3]));
          p[2] = pack2bf(fast_tanh(a1[0] + bs[1][0]), fast_tanh(a1[1] + bs[1][1]));
          p[3] = pack2bf(fast_tanh(a1[2] + bs[1][2]), fast_tanh(a1[3] + bs[1][3]));
        }
        pkd[i] = p;
        if constexpr (HEADV) {
          // the head on the bf16-ROUNDED state (the step kernel's definition): this lane's eight features in order, the node's four quads by
          // two xor-shuffles (every lane of a column ends with the same bits), the chunks in ascending order through the slot's LDS word
          // (weights, descriptor and bias are made where they are used: nothing of the head is held across the tiles, let alone the hops)
          const float4* hwp = reinterpret_cast<const float4*>(htab + chunk * 32 + q * 8);
          const float4 hw0 = hwp[0], hw1 = hwp[1];
          float ys = __builtin_bit_cast(float, p[0] << 16) * hw0.x;
          ys = __builtin_fmaf(hw0.y, __builtin_bit_cast(float, p[0] & 0xffff0000u), ys);
          ys = __builtin_fmaf(hw0.z, __builtin_bit_cast(float, p[1] << 16), ys);
          ys = __builtin_fmaf(hw0.w, __builtin_bit_cast(float, p[1] & 0xffff0000u), ys);
          ys = __builtin_fmaf(hw1.x, __builtin_bit_cast(float, p[2] << 16), ys);
          ys = __builtin_fmaf(hw1.y, __builtin_bit_cast(float, p[2] & 0xffff0000u), ys);
          ys = __builtin_fmaf(hw1.z, __builtin_bit_cast(float, p[3] << 16), ys);
          ys = __builtin_fmaf(hw1.w, __builtin_bit_cast(float, p[3] & 0xffff0000u), ys);
          ys += __shfl_xor(ys, 16, 64);
          ys += __shfl_xor(ys, 32, 64);
          if (q == 0) {
            float* yp = htab + 128 + (wave * STILES + i) * 16 + lane;      // (q == 0: lane = r)
            if (HS > 1 && chunk > 0) ys = *yp + ys;
            if (HS > 1 && !last) *yp = ys;
            if (last && node < N) {
              const __amdgpu_buffer_rsrc_t rsrc_y = __builtin_amdgcn_make_buffer_rsrc(a.y0 + ((int64_t)b * a.nsteps + step) * N, 0, N * 4, 0x00020000);
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, ys + htab[64]), rsrc_y, node * 4, 0, 0);
            }
          }
        }
        if constexpr (SCRV) {
          // chunks 0 .. HS-2 into the workgroup's scratch at the lane's SLOT (padding slots store their zeros every step: the next step reads
          // them back); the last chunk's features stay in registers and leave through the user-layout tile only
          // (RT > 0: the wave's first RT tiles stay on chip -- one 16-byte LDS store, lane-linear, read back by request_next_operand)
          if (!last) {
            if (RINGV && i < RT) *reinterpret_cast<u32x4_t*>(smem + M::RES_OFF + ((chunk * SWAVES + wave) * RT + i) * 1024 + lane * 16) = p;
            else __builtin_amdgcn_raw_buffer_store_b128(p, scratch_rsrc(), (lane & 15) * 64 + 16 * q, chunk * SCR_CH + (wave * STILES + i) * 1024, 0);
          }
        } else
        if (GCRNN_SEQ32_NT_STATE && last) __builtin_amdgcn_raw_buffer_store_b128(p, rsrc_o, node * (F * 2) + (chunk * 32 + q * 8) * 2, b * (NP * F * 2), GCRNN_SEQ32_NT_STATE);
        else __builtin_amdgcn_raw_buffer_store_b128(p, rsrc_o, node * (F * 2) + (chunk * 32 + q * 8) * 2, b * (NP * F * 2), 0);
        static_assert(!SCRV || GCRNN_SEQ32_OPERAND_AT != 3, "state scratch: the per-tile request form reads the state image");
        if (GCRNN_SEQ32_OPERAND_AT == 3 && last && more) {
          // the next operand's fragments of THIS tile (its registers died with the last tap), a tile at a time between the epilogue's own
          // work: a wave that issues all 24 requests at once sits in their issue for most of the fetch (the memory pipeline takes a request
          // when a slot frees) and does nothing else meanwhile
          const __amdgpu_buffer_rsrc_t rsrc_hn = __builtin_amdgcn_make_buffer_rsrc(hout, 0, B * (NP * F * 2), 0x00020000);
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            if (s == HS - 1) continue;
            if (s < HS)
              bfr[i][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_hn, node * (F * 2) + 16 * q + 64 * s, b * (NP * F * 2), 0));
            else
              bfr[i][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_xn, node * (G * 2) + 16 * q + 64 * (s - HS), b * (NP * G * 2), 0));
          }
        }
      }
      }
      GCRNN_STAMP32(1 + chunk * 24 + 17);
      if (!ITEMS && last) {
        // h_t's last 32 features ARE the lanes' B fragments of k-step HS-1: handed to the next step in registers
#pragma unroll
        for (int i = 0; i < STILES; ++i) bfr[i][HS - 1] = __builtin_bit_cast(bf16x8, pkd[i]);
      }
      if (GCRNN_SEQ32_OPERAND_AT == 1) request_next_operand();
      GCRNN_STAMP32(1 + chunk * 24 + 22);      // (diagnostic builds: the next operand's requests and the resident reload are issued)
      if constexpr (ITEMS) {
        // the workgroup's next item: its input was laid out by this item's pack rounds (stored, waited for and behind barriers since the
        // first half of the hops) or by the caller; its state operand is h0
        if (last && b + (int)gridDim.x < B && !GCRNN_SEQ32_NO_ITEM_PREFETCH) {
          load_first_operand(b + (int)gridDim.x);
          have_operand = true;
        }
      }
      if (aux1) {
        // user layout H[b][t][f][:] (node-contiguous rows) through a transposed LDS tile of 32-bit words [feature pair][node]: a lane's
        // four packed registers are four such words (pairs 4 q .. 4 q + 3). Nobody reads the image any more (the last hop's barrier).
        char* tst = smem;
        int swt[STILES];
        slot_words(lane, swt);
#pragma unroll
        for (int i = 0; i < STILES; ++i) {
          const int node = swt[i] >> 16;
          char* ra = tst + (4 * q) * RS2 + node * 4;
#pragma unroll
          for (int k = 0; k < 4; ++k) *reinterpret_cast<uint32_t*>(ra + k * RS2) = pkd[i][k];
        }
        lds_barrier();
        GCRNN_STAMP32(1 + chunk * 24 + 18);
      }
      // The next chunk's seed taps beside the row stores (user-layout forward, un-gated, not the step's last chunk -- its seed waits for the
      // next operand): the tap reads the resident operand, the next chunk's tap K-1 fragments (landed under hop 1's vmcnt(0) + barrier) and
      // zeroed accumulators (dead since pkd was formed) -- nothing the row stores produce, and only its `put` needs the tile to have been
      // read. As in a hop, the two waves of a SIMD take the two phases in opposite order: waves 0..3 run the 64 MFMAs while waves 4..7 drain
      // their rows (LDS reads + stores, the matrix pipe idle), then the other way round. hipcc puts s_waitcnt vmcnt(0) in front of the tap's
      // MFMAs (it places waits per block, not per path: the block is reachable from the last chunk's operand requests into the same
      // registers) -- as it did in front of the seed behind the end barrier, where all eight waves sat out the retirement of the row stores.
      // Now waves 0..3 wait for the chunk's state stores only (issued a tile phase earlier) and waves 4..7 for their own row stores while
      // waves 0..3 work. K = 2: tap 0 of the next chunk is still landing (its wait is below); the seed reads tap 1. Every wave tapping first,
      // then storing, measured 3 units more per boundary (end barrier 3.8 -> 9.6, profiles/epilogue_stamps_variants.txt).
      constexpr bool OVL = USERV && MODE == 0 && !GATED && !SPLIT;
      const bool ovl = OVL && chunk + 1 < NCH;
      if (ovl && wave < SWAVES / 2) {
        seed_taps_beside_rows(chunk + 1);
        GCRNN_STAMP32(1 + chunk * 24 + 21);
      }
      if (aux1) {
        const char* tst = smem;
        const int segs = N >> 3;
        uint16_t* ub = const_cast<uint16_t*>(aux1) + (int64_t)b * ubstride + (int64_t)(chunk * 32) * N;
        const __amdgpu_buffer_rsrc_t rsrc_u = __builtin_amdgcn_make_buffer_rsrc(ub, 0, 32 * N * 2, 0x00020000);
        // Static mapping: wave w drains feature-pair rows 2 w and 2 w + 1, a lane the 8-node segments sg = lane and lane + 64 of each (two
        // sweeps cover segs <= 128) -- no division, one base address with immediate offsets, ALL eight LDS reads of the lane in flight before
        // the first v_perm (they are inside the tile for every lane: 128 * 32 <= RS2; what lies beyond N nodes is read and never stored), and
        // every store piece in a register tuple of its own before the first store (gfx950 store-data convention). A
        // wave-instruction still stores 1 KB of contiguous bytes of one H row.
        static_assert(SWAVES * 2 == 16 && 128 * 32 <= RS2, "row stores: two feature-pair rows per wave, two sweeps of 64 segments inside a tile row");
        const int ln = lane_now();
        const char* rb = tst + (2 * wave) * RS2 + ln * 32;
        u32x4_t rw[4][2], rv[4][2];
#pragma unroll
        for (int p = 0; p < 4; ++p) {      // piece p: row 2 w + (p & 1), sweep p >> 1
          rw[p][0] = *reinterpret_cast<const u32x4_t*>(rb + (p & 1) * RS2 + (p >> 1) * 2048);
          rw[p][1] = *reinterpret_cast<const u32x4_t*>(rb + (p & 1) * RS2 + (p >> 1) * 2048 + 16);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const u32x4_t w0 = rw[p][0], w1 = rw[p][1];
          rv[p][0] = u32x4_t{__builtin_amdgcn_perm(w0[1], w0[0], 0x05040100u), __builtin_amdgcn_perm(w0[3], w0[2], 0x05040100u),
                             __builtin_amdgcn_perm(w1[1], w1[0], 0x05040100u), __builtin_amdgcn_perm(w1[3], w1[2], 0x05040100u)};
          rv[p][1] = u32x4_t{__builtin_amdgcn_perm(w0[1], w0[0], 0x07060302u), __builtin_amdgcn_perm(w0[3], w0[2], 0x07060302u),
                             __builtin_amdgcn_perm(w1[1], w1[0], 0x07060302u), __builtin_amdgcn_perm(w1[3], w1[2], 0x07060302u)};
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) { asm volatile("" : "+v"(rv[p][0])); asm volatile("" : "+v"(rv[p][1])); }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int fp = 2 * wave + (p & 1), sg = ln + 64 * (p >> 1);
          if (sg < segs) {
            __builtin_amdgcn_raw_buffer_store_b128(rv[p][0], rsrc_u, ((2 * fp) * N + sg * 8) * 2, 0, GCRNN_SEQ32_NT_ROWS);
            __builtin_amdgcn_raw_buffer_store_b128(rv[p][1], rsrc_u, ((2 * fp + 1) * N + sg * 8) * 2, 0, GCRNN_SEQ32_NT_ROWS);
          }
        }
      }
      if (ovl && wave >= SWAVES / 2) seed_taps_beside_rows(chunk + 1);
      // this chunk's stores have retired (the next step reads some of them back; K = 2: the next chunk's tap 0 has landed), the tile
      // has been read: the image may be seeded again
      if (GCRNN_SEQ32_OPERAND_AT == 2) request_next_operand();
      GCRNN_STAMP32(1 + chunk * 24 + 19);
      // K = 2 only: the next chunk's tap 0 (LDS-DMA behind the last hop) has landed. Otherwise NO wait here: every LDS-DMA piece was covered by
      // its hop's wait, the stores the next step reads back (the earlier chunks' states, the pack's rows) have been behind a hop's vmcnt(0)
      // since, and the next operand's requests are waited for where the seed's MFMAs first use them (hipcc counts them: the state fragments
      // were requested first, so the seed starts on them while the input's are still landing).
      if (K == 2 && NCH > 1 && !SPLIT && !RINGV) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (GCRNN_SEQ32_END_WAIT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();
      GCRNN_STAMP32(1 + chunk * 24 + 20);
      if (!SPLIT && chunk + 1 < NCH) {
        if (ovl) put(std::false_type{});      // (its taps ran beside the row stores)
        else seed(chunk + 1);
      }
    }  // chunks
  }  // steps
  }  // sequences
  GCRNN_STAMP32_FLUSH();
}
