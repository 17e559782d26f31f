// gemm_x6.hip -- fp32-accurate row-major GEMM  C[M][N] (+)= A[M][K] . W[N][K]^T + bias  on the bf16 matrix cores of gfx950:
// the linear layers of the s2mel DiT / WaveNet (row N1 of SURVEY.md 8(f)): `Attention.wqkv / wo`, `FeedForward.w1|w3 / w2`
// (indextts/s2mel/modules/gpt_fast/model.py:242-326), the WaveNet's k = 5 convs as five row-shifted GEMMs and its 1x1
// res / skip convs (wavenet.py:103-174), the AdaLN projections and the merge / skip linears (diffusion_transformer.py:186-257).
//
// Arithmetic: every fp32 product as six exact bf16 partial products with fp32 accumulation (conv1d_x3.hip's scheme):
// x = h + m + l, each piece the remainder before it rounded to 8 significant bits; hh' hm' mh' mm' hl' lh' carry x.w to 2^-24.
//
// What the r02 attempt (128 x 128 tiles, operand fragments straight from L2) lost on was operand bytes per MFMA.  Here both operands
// go through LDS, shared by the four waves of a 256 x 128 / 128 x 128 tile:
//   * the WEIGHTS are split once at load (`ixtts_gemm_x6_pack`) into planes [k/16][plane 3][k-half 2][N_pad] of 16-byte units
//     (eight consecutive k of one output feature = the B operand of a lane);
//   * the ACTIVATIONS are split into the same layout [k/16][3][2][M_pad] by a small pass (`ixtts_gemm_x6_split`: one coalesced read of
//     the fp32 rows, 6 B per element written) -- a producer that writes the planes itself saves that pass (the AdaLN norm in front
//     of [w1; w3] does: dit_ops.hip, `ixtts_adaln_rmsnorm_planes_f32`);
//   * both are copied global -> LDS by LDS-DMA into a 4-stage ring, THREE 16-deep steps ahead of the MFMAs: with one step of cover
//     (the first version) every barrier waited out a full L2 / Infinity-Cache round trip and the kernel ran at the library's speed;
//   * the blockIdx -> tile map gives each XCD a contiguous run of tiles, row-tile major: the tiles of one XCD share their A rows in
//     its L2.
// MFMA operands: A = activations (lane: row l & 31, k-half l >> 5), B = weights (lane: output feature l & 31, k-half l >> 5), so an
// accumulator register holds 32 CONSECUTIVE output features of one row: the epilogue's stores are 128-byte row segments.
#include "common.h"

namespace ixtts {

typedef float gx_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 gx_bf16x8 __attribute__((ext_vector_type(8)));
typedef float gx_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int gx_u32x4 __attribute__((ext_vector_type(4)));


// fp32 [N][K] -> packed planes [K/16][3][2][N_pad] units; rows n >= N are zero
__global__ void gemm_x6_pack_kernel(const float* __restrict__ w, uint4* __restrict__ out, int N, int K, int Npad) {
  const long total = (long)(K / 8) * Npad;  // one thread per (k-octet, n)
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int n = (int)(idx % Npad);
    const int ko = (int)(idx / Npad);  // k-octet: g = ko / 2, kh = ko % 2
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = n < N ? w[(long)n * K + ko * 8 + e] : 0.f;
    uint4 ph, pm, pl;
    split8_bf16x3(v, ph, pm, pl);
    const int g = ko >> 1, kh = ko & 1;
    uint4* base = out + ((long)g * 6) * Npad + n;
    base[(long)(0 * 2 + kh) * Npad] = ph;
    base[(long)(1 * 2 + kh) * Npad] = pm;
    base[(long)(2 * 2 + kh) * Npad] = pl;
  }
}

// Activations A [M][K] (row stride lda) -> the same packed planes [K/16][3][2][Mpad] units, rows >= M zero.  One workgroup = 64 rows x
// 64 k: coalesced 256-byte row reads into an LDS tile, then one (row, k-octet) unit per thread and plane, rows contiguous across lanes.
// HALO (the WaveNet's reflect-padded row buffers): a halo row is read from the interior row that `reflect_halo_rows_kernel` would have
// copied into it, so the planes equal halo refresh + split without the refresh.  1: sequences of hleft + hT + hright rows back to back;
// 2: packed, sequence s = rows [hoff[s], hoff[s+1]) with its own halo rows (one too short to reflect is read as it is, as the refresh
// leaves it).
template <int HALO>
__device__ __forceinline__ long split_src_row(long rr, int hT, int hleft, int hright, const int* __restrict__ hoff, int hn) {
  if constexpr (HALO == 0) return rr;
  long o0;
  int T = hT;
  if constexpr (HALO == 1) {
    o0 = rr / (hleft + hT + hright) * (hleft + hT + hright);
  } else {
    const int s = seq_of_row(hoff, hn, rr);
    o0 = hoff[s];
    T = hoff[s + 1] - (int)o0 - hleft - hright;
    if (T <= hleft || T <= hright) return rr;
  }
  const int h = (int)(rr - o0);
  if (h < hleft) return o0 + 2 * hleft - h;                          // halo row hleft-1-i <- interior row i+1
  if (h >= hleft + T && h < hleft + T + hright) return o0 + 2 * (hleft + T) - 2 - h;  // halo row hleft+T+i <- interior row T-2-i
  return rr;
}

template <int HALO = 0>
__global__ __launch_bounds__(256) void gemm_x6_split_kernel(const float* __restrict__ a, long lda, uint4* __restrict__ out, int M, int K, long Mpad, int hT = 0,
                                                            int hleft = 0, int hright = 0, const int* __restrict__ hoff = nullptr, int hn = 0) {
  __shared__ float tile[64][65];
  const int r0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (t >> 4) + 16 * i, kq = t & 15;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < M) v = *reinterpret_cast<const float4*>(a + split_src_row<HALO>(r0 + r, hT, hleft, hright, hoff, hn) * lda + k0 + 4 * kq);
    tile[r][4 * kq + 0] = v.x; tile[r][4 * kq + 1] = v.y; tile[r][4 * kq + 2] = v.z; tile[r][4 * kq + 3] = v.w;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r = t & 63, o = (t >> 6) + 4 * u;  // k-octet of this 64-wide k block
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tile[r][o * 8 + e];
    uint4 ph, pm, pl;
    split8_bf16x3(v, ph, pm, pl);
    const int ko = (k0 >> 3) + o, g = ko >> 1, kh = ko & 1;
    uint4* base = out + ((long)g * 6) * Mpad + r0 + r;
    base[(long)(0 * 2 + kh) * Mpad] = ph;
    base[(long)(1 * 2 + kh) * Mpad] = pm;
    base[(long)(2 * 2 + kh) * Mpad] = pl;
  }
}

// Epilogues.  The pair forms read the weights packed with their two halves interleaved in 32-row blocks (block 2q = rows
// [32q, 32q + 32) of the first half, block 2q + 1 the same rows of the second), so one wave's two 32-column accumulator blocks hold
// matching columns a, b of the two halves and the tile writes N / 2 columns: output column 32q + l31.
enum { EPI_PLAIN = 0, EPI_SWIGLU = 1, EPI_GATE = 2 };  // C (+)= acc + bias  |  silu(a) * b  |  tanh(a + g_a) * sigmoid(b + g_b)

struct GemmX6Params {
  const uint4* Ap;   // activation planes [K/16][6][Mpad], this GEMM's rows start at unit `arow0`
  long Mpad;
  long arow0;
  const uint4* Wp;   // weight planes [K/16][6][Npad]
  const float* bias;
  float* C;
  long ldc;
  int M, N, Npad, K, accumulate, m_tiles, n_tiles;
  int tap_steps;     // 16-deep steps per tap: step s reads k-group s % tap_steps of the planes, rows shifted down by s / tap_steps
  int epi;           // EPI_*: what the tile writes
  const float* gate; // EPI_GATE: per-batch gate biases, row r takes gate[min(r / rows_per_batch, nbatch - 1) * gate_ld + ...]
  long gate_ld, rows_per_batch;
  int nbatch;
  const int* gate_seq_off;  // EPI_GATE over packed sequences: row r takes the gate of the s with off[s] <= r < off[s+1] (nbatch = n), or null
  unsigned long long* dbg;  // DBG == 3: per-step phase stamps of workgroup 0, wave 0 (developer timing)
};


// C tile BM x BN = (64 MT) x (64 NT), 4 waves as 2 x 2.  Both operands arrive as bf16 planes and are copied global -> LDS by LDS-DMA
// into a 4-stage ring, three 16-deep steps ahead; every memory operation of the main loop is issued by hand (DMA builtins, fragment
// reads from ONE asm block that ends in its own wait), so the only vmcnt waits are the counted ones below: left to the compiler, a
// ds_read of a stage that a copy of an earlier loop iteration filled drains every copy in flight (vmcnt(0)) -- it cannot count across
// the back edge.
// NST LDS stages: the operand copies run NST - 1 steps ahead of the MFMAs.  DBG (developer timing, results meaningless): 1 = no operand
// copies in the main loop, 2 = no fragment reads / MFMAs, 3 = phase stamps.
// The epilogue is chosen at compile time: EPI (EPI_*), ACC (EPI_PLAIN: C += ...), SEQ (EPI_GATE: gate row by the sequence table
// p.gate_seq_off instead of row / rows_per_batch); `run_gemm_x6` dispatches on p.epi / p.accumulate / p.gate_seq_off.
// PIN: 1 = a step's MFMAs are fenced ahead of its closing wait and barrier (developer A/B, tiles 42 / 43); 0 = the scheduler places
// them, which measured 1-2 % faster on both production kernels (profiles/r07_notes.md).
// PIPE: 1 = the pipelined main loop (tile 6; 128 x 128, 4 stages, one workgroup per CU): a second fragment set in registers and the
// copies spread through the MFMAs, for grids of no more tiles than CUs, where no second workgroup hides a wave's issue cycles
// (profiles/r14_notes.md).  0 = the loop described above, instruction for instruction what it was before PIPE existed.
template <int MT, int NT, int NST, int EPI = EPI_PLAIN, int ACC = 0, int SEQ = 0, int DBG = 0, int PIN = 0, int PIPE = 0>
__global__ __launch_bounds__(256, (NST * (MT + NT) * 6 * 64 * 16 <= 80 * 1024) ? 2 : 1) void gemm_x6_kernel(GemmX6Params p) {
  constexpr int BM = 64 * MT, BN = 64 * NT;
  constexpr int A_UNITS = 6 * BM, W_UNITS = 6 * BN, STAGE = A_UNITS + W_UNITS;
  constexpr int NDMA = (6 * (MT + NT)) / 4;       // LDS-DMA instructions per wave and step
  constexpr int NA = (6 * MT) / 4, NW = NDMA - NA;  // of which the first NA copy A pieces and the rest W pieces, in every wave
  static_assert((6 * MT) % 4 == 0 && (6 * NT) % 4 == 0, "the A pieces and the W pieces are each dealt evenly to the 4 waves");
  static_assert(EPI == EPI_PLAIN || (ACC == 0 && NT == 2), "pair epilogues: the wave's two 32-column blocks are the two halves");
  static_assert(EPI == EPI_GATE || SEQ == 0, "the sequence table belongs to the gate epilogue");
  constexpr int D = NST - 1;                      // steps the copies run ahead
  extern __shared__ uint4 smem[];                 // NST stages x [A image [3][2][BM] | W image [3][2][BN]]

  // ---- XCD-aware tile id: blocks b and b + 8 share an XCD; each XCD takes a contiguous run of tiles, row-tile major
  const int nwg = p.m_tiles * p.n_tiles;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, idx = bid >> 3;
  const int qd = nwg >> 3, rm = nwg & 7;
  const int lin = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + idx;
  const int m_tile = lin / p.n_tiles, n_tile = lin - m_tile * p.n_tiles;
  const int m0 = m_tile * BM, n0 = n_tile * BN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform to the compiler too: what depends on it stays in SGPRs
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;

  gx_f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // one step's copies: 6 runs (plane, k-half) of BM + BN units, in pieces of 64 units (one LDS-DMA wave-instruction each)
  // Piece e = q * 4 + wave of the step's 6 (MT + NT): the A pieces come first and 6 MT is a multiple of 4, so a wave's copies q < NA
  // are A pieces and the others W pieces.  Step s reads A at k-group s % tap_steps of the planes, rows shifted down by s / tap_steps,
  // and W at k-group s: both affine in s, so each piece's source (at step 0) and LDS offset are fixed here and a step's copy is that
  // source plus one running offset, uniform over the wave.
  const uint4* asrc = p.Ap + p.arow0 + m0 + lane;
  const uint4* wsrc = p.Wp + n0 + lane;
  long a_off[NA], w_off[NW];  // units
  int a_lds[NA], w_lds[NW];
#pragma unroll
  for (int q = 0; q < NA; ++q) {
    const int e = q * 4 + wave, run = e / MT, piece = e % MT;
    a_off[q] = run * p.Mpad + piece * 64;
    a_lds[q] = run * BM + piece * 64;
  }
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const int e = q * 4 + wave, run = e / NT, piece = e % NT;
    w_off[q] = (long)run * p.Npad + piece * 64;
    w_lds[q] = A_UNITS + run * BN + piece * 64;
  }
  const long a_step = 6 * p.Mpad, w_step = 6L * p.Npad;
  const long a_wrap = 1 - p.tap_steps * a_step;  // after the last k-group of a tap: back to k-group 0, one row down
  long a_run = 0, w_run = 0;                      // the next step's offsets
  int a_group = 0;                                // and its k-group within the tap
  // STATEFUL: the k-th call issues the copies of step k.  The prologue calls it for steps 0 .. D - 1 and main-loop step s for step
  // s + D, in that order and with none left out (DBG == 1 stops after the prologue).  It is `issue_piece` for the wave's pieces
  // q = 0 .. NDMA - 1 and then `issue_advance`; the pipelined loop (PIPE) makes those calls itself, one piece every few MFMAs.
  auto issue_piece = [&](uint4* st, int q) {
    if (q < NA)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc + (a_off[q] + a_run)),
                                       (__attribute__((address_space(3))) void*)(st + a_lds[q]), 16, 0, 0);
    else
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc + (w_off[q - NA] + w_run)),
                                       (__attribute__((address_space(3))) void*)(st + w_lds[q - NA]), 16, 0, 0);
  };
  auto issue_advance = [&]() {
    a_run += a_step;
    w_run += w_step;
    if (++a_group == p.tap_steps) {
      a_group = 0;
      a_run += a_wrap;
    }
  };
  auto issue_next = [&](uint4* st) {
#pragma unroll
    for (int q = 0; q < NDMA; ++q) issue_piece(st, q);
    issue_advance();
  };

  const int steps = p.K >> 4;
  auto wg_stamp = [&](int k) {  // DBG == 3: per-workgroup wall clock (100 MHz) at entry / loop start / loop end / exit, behind the step stamps
    if constexpr (DBG == 3) {
      if (tid == 0) p.dbg[128 + (long)blockIdx.x * 4 + k] = __builtin_amdgcn_s_memrealtime();
    }
  };
  // counted wait: leave the copies of the `y` youngest steps in flight (vmcnt counts in order)
  auto wait_younger = [&](int y) {
    if (y >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NDMA) : "memory");
    else if (y == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  static_assert(D >= 1 && D <= 3, "1..3 steps of copies in flight behind the one waited for");
  wg_stamp(0);
  if constexpr (PIPE != 0) {
    // PIPELINED LOOP (tile 6).  One workgroup per CU and one wave per SIMD: nothing else hides this wave's issue cycles, so the
    // fragment reads of step s + 1 and the copies of step s + D are issued AMONG the 24 MFMAs of step s.  The fragments are double-
    // buffered in registers: step s multiplies set s & 1 while the reads of step s + 1 fill the other set.  Stage of step t: t % NST.
    // Step s, in order:  [MFMAs of step s on set s & 1, and among them: the read block of step s + 1 into set (s + 1) & 1, then the
    // wave's NDMA copies of step s + D]  ->  lgkmcnt(0) (the reads have arrived; they take the set as "+v" operands, so the compiler
    // can neither read nor move those registers across the wait)  ->  counted vmcnt (this wave's share of step s + 2's copies has
    // landed; those of step s + 3 stay in flight)  ->  barrier.
    // (a) Reads only see landed data: step s + 1's read block runs in step s, behind the barrier that closes step s - 1 (for s = 0:
    //     the prologue's), in front of which every wave waited until its share of step s + 1's copies had landed.
    // (b) A copy never overwrites a stage in use: step s's copies go to stage (s + D) % NST = (s - 1) % NST with D = NST - 1 = 3 --
    //     neither the stage read in step s, (s + 1) % NST, nor the one read in step s + 1, (s + 2) % NST.  Its last reader was the
    //     read block of step s - 1, issued in step s - 2 and waited for (lgkmcnt(0)) in front of the barrier that closes step s - 2.
    // (c) Short runs: K is a multiple of 64 (checked at every entry), so steps is a multiple of 4 and >= 4 = D + 1.  The loop below
    //     takes the steps that both read ahead and copy ahead in pairs (the register sets alternate); the last four steps are
    //     written out: steps - 4 issues the last copies (of step steps - 1), steps - 3 waits for all of them, steps - 2 reads the
    //     last step and needs no barrier (nothing is copied or read from LDS after it), steps - 1 only multiplies.  No read of a
    //     step that does not exist, no wait for copies never issued.
    // For every accumulator the MFMA order is the other loop's: steps in order, al.bh ah.bl am.bm am.bh ah.bm ah.bh within a step.
    static_assert(MT == 2 && NT == 2 && NST == 4 && PIN == 0 && (DBG == 0 || DBG == 3), "the pipelined loop: 128 x 128 tile, 4 stages");
    static_assert(D % NST != 0 && D % NST != 1 % NST && D % NST != 2 % NST, "(b): the copy target is none of the stages of steps s, s + 1, s + 2");
    constexpr int RD_AT = 1, CP_AT = 2, CP_EVERY = 3;  // the read block follows MFMA RD_AT of the step's 24, copy q MFMA CP_AT + q CP_EVERY
    static_assert(RD_AT < CP_AT && CP_AT + (NDMA - 1) * CP_EVERY < 6 * MT * NT, "reads, then the copies, all among the step's MFMAs");
    const unsigned base_addr = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)smem;
    const unsigned a_rel = (unsigned)((lh * BM + wm * (32 * MT) + l31) * 16), w_rel = (unsigned)((A_UNITS + lh * BN + wn * (32 * NT) + l31) * 16);
    gx_u32x4 fa[2][3][MT], fb[2][3][NT];  // [set][plane][i or j]; the set index is a compile-time constant everywhere
    // the 12 fragment reads of one step (stage `stage`) into one set (a, b): issued, NOT waited for
    auto read_issue = [&](gx_u32x4 (&a)[3][MT], gx_u32x4 (&b)[3][NT], int stage) {
      const unsigned aaddr = base_addr + (unsigned)(stage * STAGE * 16) + a_rel, waddr = base_addr + (unsigned)(stage * STAGE * 16) + w_rel;
      asm volatile(
          "ds_read_b128 %0, %12 offset:%14\n ds_read_b128 %1, %12 offset:%15\n ds_read_b128 %2, %12 offset:%16\n ds_read_b128 %3, %12 offset:%17\n"
          "ds_read_b128 %4, %12 offset:%18\n ds_read_b128 %5, %12 offset:%19\n ds_read_b128 %6, %13 offset:%20\n ds_read_b128 %7, %13 offset:%21\n"
          "ds_read_b128 %8, %13 offset:%22\n ds_read_b128 %9, %13 offset:%23\n ds_read_b128 %10, %13 offset:%24\n ds_read_b128 %11, %13 offset:%25"
          : "=&v"(a[0][0]), "=&v"(a[0][1]), "=&v"(a[1][0]), "=&v"(a[1][1]), "=&v"(a[2][0]), "=&v"(a[2][1]), "=&v"(b[0][0]),
            "=&v"(b[0][1]), "=&v"(b[1][0]), "=&v"(b[1][1]), "=&v"(b[2][0]), "=&v"(b[2][1])
          : "v"(aaddr), "v"(waddr), "n"((0 * 2 * BM + 0) * 16), "n"((0 * 2 * BM + 32) * 16), "n"((1 * 2 * BM + 0) * 16), "n"((1 * 2 * BM + 32) * 16),
            "n"((2 * 2 * BM + 0) * 16), "n"((2 * 2 * BM + 32) * 16), "n"((0 * 2 * BN + 0) * 16), "n"((0 * 2 * BN + 32) * 16), "n"((1 * 2 * BN + 0) * 16),
            "n"((1 * 2 * BN + 32) * 16), "n"((2 * 2 * BN + 0) * 16), "n"((2 * 2 * BN + 32) * 16)
          : "memory");
    };
    // ... and the wait that makes that set usable: the data dependency of everything that reads the set runs through this statement
    auto read_wait = [&](gx_u32x4 (&a)[3][MT], gx_u32x4 (&b)[3][NT]) {
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[2][0]), "+v"(a[2][1]), "+v"(b[0][0]),
                     "+v"(b[0][1]), "+v"(b[1][0]), "+v"(b[1][1]), "+v"(b[2][0]), "+v"(b[2][1])
                   :
                   : "memory");
    };
    auto stamp = [&](int s, int k) {
      if constexpr (DBG == 3) {
        if (blockIdx.x == 0 && tid == 0 && s < 16) {
          p.dbg[s * 8 + k] = __builtin_amdgcn_s_memtime();
          if (k == 0) p.dbg[s * 8 + 7] = __builtin_amdgcn_s_memrealtime();
        }
      }
    };
    int st_rd = 1, st_cp = D % NST;  // stages of step s + 1 (read in step s) and of step s + D (copied in step s)
    // one step on set c.  COPY: step s + D exists; READ: step s + 1 exists; SYNC: a later step still reads LDS
    auto step = [&](auto set, auto copy, auto read, auto sync, int s) {
      constexpr int c = decltype(set)::value;
      constexpr bool COPY = decltype(copy)::value, READ = decltype(read)::value, SYNC = decltype(sync)::value;
      static_assert(READ || !COPY, "copies are only issued for steps that will be read");
      static_assert(READ || !SYNC, "the closing wait and barrier publish data to a later read block");
      stamp(s, 0);
      if constexpr (DBG == 3) __builtin_amdgcn_sched_barrier(0);
      uint4* const cp_stage = smem + st_cp * STAGE;
      auto among = [&](int k) {  // what follows MFMA k of the step (k is a constant once the loops below are unrolled)
        if (READ && k == RD_AT) {
          __builtin_amdgcn_sched_barrier(0);
          read_issue(fa[1 - c], fb[1 - c], st_rd);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (COPY && k >= CP_AT && (k - CP_AT) % CP_EVERY == 0 && (k - CP_AT) / CP_EVERY < NDMA) {
          __builtin_amdgcn_sched_barrier(0);
          issue_piece(cp_stage, (k - CP_AT) / CP_EVERY);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const gx_bf16x8 ah = __builtin_bit_cast(gx_bf16x8, fa[c][0][i]), am = __builtin_bit_cast(gx_bf16x8, fa[c][1][i]), al = __builtin_bit_cast(gx_bf16x8, fa[c][2][i]);
          const gx_bf16x8 bh = __builtin_bit_cast(gx_bf16x8, fb[c][0][j]), bm = __builtin_bit_cast(gx_bf16x8, fb[c][1][j]), bl = __builtin_bit_cast(gx_bf16x8, fb[c][2][j]);
          const int k0 = (i * NT + j) * 6;
          // smallest partial products first
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[i][j], 0, 0, 0);
          among(k0 + 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[i][j], 0, 0, 0);
          among(k0 + 1);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc[i][j], 0, 0, 0);
          among(k0 + 2);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[i][j], 0, 0, 0);
          among(k0 + 3);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[i][j], 0, 0, 0);
          among(k0 + 4);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[i][j], 0, 0, 0);
          among(k0 + 5);
        }
      if constexpr (COPY) issue_advance();
      if constexpr (DBG == 3) asm volatile("" ::"v"(acc[0][0][0]), "v"(acc[MT - 1][NT - 1][15]));  // (the stamp below sits behind the last MFMAs' results)
      stamp(s, 1);
      if constexpr (READ) read_wait(fa[1 - c], fb[1 - c]);
      stamp(s, 2);
      if constexpr (SYNC) {
        wait_younger(COPY ? 1 : 0);
        stamp(s, 3);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      } else {
        stamp(s, 3);
      }
      stamp(s, 4);
      st_rd = (st_rd + 1) & (NST - 1);
      st_cp = (st_cp + 1) & (NST - 1);
    };
    constexpr std::integral_constant<int, 0> S0;
    constexpr std::integral_constant<int, 1> S1;
    constexpr std::true_type Y;
    constexpr std::false_type N_;

    for (int t = 0; t < D; ++t) issue_next(smem + t * STAGE);  // steps 0 .. D - 1 (steps >= D + 1)
    wait_younger(1);  // steps 0 and 1 have landed, step 2 stays in flight
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    read_issue(fa[0], fb[0], 0);
    read_wait(fa[0], fb[0]);
    wg_stamp(1);
    int s = 0;
    for (; s + 4 < steps; s += 2) {
      step(S0, Y, Y, Y, s);
      step(S1, Y, Y, Y, s + 1);
    }
    step(S0, Y, Y, Y, s);         // steps - 4: the last copies
    step(S1, N_, Y, Y, s + 1);    // steps - 3: waits for them
    step(S0, N_, Y, N_, s + 2);   // steps - 2: the last reads
    step(S1, N_, N_, N_, s + 3);  // steps - 1: multiplies only
  } else {
    for (int t = 0; t < D && t < steps; ++t) issue_next(smem + t * STAGE);  // steps 0 .. D - 1
    wait_younger(min(D, steps) - 1);  // step 0's copies (the oldest) have landed
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    wg_stamp(1);

    // Step s computes on stage s % NST and, first, issues the copies of step s + D into stage (s + D) % NST (last read in step s - 1,
    // which every wave has left).  Before its closing barrier a wave waits until its share of step s + 1's copies has landed; the
    // copies of the steps behind that stay in flight.  Every memory operation here is issued by hand, so a run-time stage index and
    // run-time issue condition are fine: the compiler has no wait of its own to miscount.
    const unsigned base_addr = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)smem;
    int st_cur = 0, st_nxt = D % NST;
    for (int s = 0; s < steps; ++s) {
      auto stamp = [&](int k) {
        if constexpr (DBG == 3) {
          if (blockIdx.x == 0 && tid == 0 && s < 16) {
            p.dbg[s * 8 + k] = __builtin_amdgcn_s_memtime();
            if (k == 0) p.dbg[s * 8 + 7] = __builtin_amdgcn_s_memrealtime();
          }
        }
      };
      stamp(0);
      if (DBG != 1 && s + D < steps) issue_next(smem + st_nxt * STAGE);  // step s + D
      stamp(1);
      const unsigned cur_addr = base_addr + (unsigned)(st_cur * STAGE * 16);
      if constexpr (DBG != 2) {
        // fragments: A [plane][i] at unit (plane * 2 + lh) * BM + wm * 32 MT + i * 32 + l31; W likewise behind the A image
        gx_u32x4 af[3][MT], bf[3][NT];
        const unsigned aaddr = cur_addr + (unsigned)((lh * BM + wm * (32 * MT) + l31) * 16);
        const unsigned waddr = cur_addr + (unsigned)((A_UNITS + lh * BN + wn * (32 * NT) + l31) * 16);
        if constexpr (MT == 4 && NT == 2) {
          asm volatile(
              "ds_read_b128 %0, %18 offset:%20\n ds_read_b128 %1, %18 offset:%21\n ds_read_b128 %2, %18 offset:%22\n ds_read_b128 %3, %18 offset:%23\n"
              "ds_read_b128 %4, %18 offset:%24\n ds_read_b128 %5, %18 offset:%25\n ds_read_b128 %6, %18 offset:%26\n ds_read_b128 %7, %18 offset:%27\n"
              "ds_read_b128 %8, %18 offset:%28\n ds_read_b128 %9, %18 offset:%29\n ds_read_b128 %10, %18 offset:%30\n ds_read_b128 %11, %18 offset:%31\n"
              "ds_read_b128 %12, %19 offset:%32\n ds_read_b128 %13, %19 offset:%33\n ds_read_b128 %14, %19 offset:%34\n ds_read_b128 %15, %19 offset:%35\n"
              "ds_read_b128 %16, %19 offset:%36\n ds_read_b128 %17, %19 offset:%37\n s_waitcnt lgkmcnt(0)"
              : "=&v"(af[0][0]), "=&v"(af[0][1]), "=&v"(af[0][2]), "=&v"(af[0][3]), "=&v"(af[1][0]), "=&v"(af[1][1]), "=&v"(af[1][2]), "=&v"(af[1][3]),
                "=&v"(af[2][0]), "=&v"(af[2][1]), "=&v"(af[2][2]), "=&v"(af[2][3]), "=&v"(bf[0][0]), "=&v"(bf[0][1]), "=&v"(bf[1][0]), "=&v"(bf[1][1]),
                "=&v"(bf[2][0]), "=&v"(bf[2][1])
              : "v"(aaddr), "v"(waddr), "n"((0 * 2 * BM + 0) * 16), "n"((0 * 2 * BM + 32) * 16), "n"((0 * 2 * BM + 64) * 16), "n"((0 * 2 * BM + 96) * 16),
                "n"((1 * 2 * BM + 0) * 16), "n"((1 * 2 * BM + 32) * 16), "n"((1 * 2 * BM + 64) * 16), "n"((1 * 2 * BM + 96) * 16), "n"((2 * 2 * BM + 0) * 16),
                "n"((2 * 2 * BM + 32) * 16), "n"((2 * 2 * BM + 64) * 16), "n"((2 * 2 * BM + 96) * 16), "n"((0 * 2 * BN + 0) * 16), "n"((0 * 2 * BN + 32) * 16),
                "n"((1 * 2 * BN + 0) * 16), "n"((1 * 2 * BN + 32) * 16), "n"((2 * 2 * BN + 0) * 16), "n"((2 * 2 * BN + 32) * 16)
              : "memory");
        } else {
          static_assert(MT == 2 && NT == 2, "fragment block written for 256 x 128 and 128 x 128 tiles");
          asm volatile(
              "ds_read_b128 %0, %12 offset:%14\n ds_read_b128 %1, %12 offset:%15\n ds_read_b128 %2, %12 offset:%16\n ds_read_b128 %3, %12 offset:%17\n"
              "ds_read_b128 %4, %12 offset:%18\n ds_read_b128 %5, %12 offset:%19\n ds_read_b128 %6, %13 offset:%20\n ds_read_b128 %7, %13 offset:%21\n"
              "ds_read_b128 %8, %13 offset:%22\n ds_read_b128 %9, %13 offset:%23\n ds_read_b128 %10, %13 offset:%24\n ds_read_b128 %11, %13 offset:%25\n"
              "s_waitcnt lgkmcnt(0)"
              : "=&v"(af[0][0]), "=&v"(af[0][1]), "=&v"(af[1][0]), "=&v"(af[1][1]), "=&v"(af[2][0]), "=&v"(af[2][1]), "=&v"(bf[0][0]), "=&v"(bf[0][1]),
                "=&v"(bf[1][0]), "=&v"(bf[1][1]), "=&v"(bf[2][0]), "=&v"(bf[2][1])
              : "v"(aaddr), "v"(waddr), "n"((0 * 2 * BM + 0) * 16), "n"((0 * 2 * BM + 32) * 16), "n"((1 * 2 * BM + 0) * 16), "n"((1 * 2 * BM + 32) * 16),
                "n"((2 * 2 * BM + 0) * 16), "n"((2 * 2 * BM + 32) * 16), "n"((0 * 2 * BN + 0) * 16), "n"((0 * 2 * BN + 32) * 16), "n"((1 * 2 * BN + 0) * 16),
                "n"((1 * 2 * BN + 32) * 16), "n"((2 * 2 * BN + 0) * 16), "n"((2 * 2 * BN + 32) * 16)
              : "memory");
        }
        stamp(2);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            const gx_bf16x8 ah = __builtin_bit_cast(gx_bf16x8, af[0][i]), am = __builtin_bit_cast(gx_bf16x8, af[1][i]), al = __builtin_bit_cast(gx_bf16x8, af[2][i]);
            const gx_bf16x8 bh = __builtin_bit_cast(gx_bf16x8, bf[0][j]), bm = __builtin_bit_cast(gx_bf16x8, bf[1][j]), bl = __builtin_bit_cast(gx_bf16x8, bf[2][j]);
            // smallest partial products first
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[i][j], 0, 0, 0);
          }
        if constexpr (DBG == 3) asm volatile("" ::"v"(acc[0][0][0]), "v"(acc[MT - 1][NT - 1][15]));  // (the stamp below sits behind the last MFMAs' results)
        // The MFMAs touch registers only, so nothing orders them against the wait below and the scheduler may put the wait and the
        // barrier in front of some of them.  Fencing them here was timed and lost (the CU's other workgroup keeps the matrix pipe fed).
        if constexpr (PIN != 0) __builtin_amdgcn_sched_barrier(0);
      }
      stamp(3);
      wait_younger(DBG == 1 ? 0 : max(0, min(D - 1, steps - s - 2)));
      stamp(4);
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      stamp(5);
      st_cur = st_cur + 1 == NST ? 0 : st_cur + 1;
      st_nxt = st_nxt + 1 == NST ? 0 : st_nxt + 1;
    }
  }

  wg_stamp(2);
  // ---- epilogue: register r of a lane = row (r & 3) + 8 (r >> 2) + 4 lh of the 32 x 32 tile, column l31
  if constexpr (EPI != EPI_PLAIN) {
    const int oc = (n0 + wn * 64) / 2 + l31;  // output column
    const int nh = p.N >> 1;
    if (oc < nh) {
      // rows and batch sizes are below 2^31 (a larger rows_per_batch gives batch 0 either way): one 32-bit division per element
      // where the 64-bit one was some 230 instructions, 32 times per lane
      const unsigned rpb = (unsigned)min(p.rows_per_batch, (long)0x7fffffff);
      const float ba = p.bias != nullptr ? p.bias[n0 + wn * 64 + l31] : 0.f, bb = p.bias != nullptr ? p.bias[n0 + wn * 64 + 32 + l31] : 0.f;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int rbase = m0 + wm * (32 * MT) + i * 32 + 4 * lh;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rbase + (r & 3) + 8 * (r >> 2);
          if (row < p.M) {
            float a = acc[i][0][r] + ba, b = acc[i][1][r] + bb, v;
            if constexpr (EPI == EPI_SWIGLU) {
              v = a / (1.0f + expf(-a)) * b;  // swiglu_kernel's arithmetic
            } else {
              long gb;
              if constexpr (SEQ != 0) gb = (long)seq_of_row(p.gate_seq_off, p.nbatch, row);
              else gb = min((long)((unsigned)row / rpb), (long)p.nbatch - 1);
              const float* g = p.gate + gb * p.gate_ld;
              a += g[oc];
              b += g[nh + oc];
              v = tanhf(a) * (1.0f / (1.0f + expf(-b)));  // wn_gate_rows_kernel's arithmetic
            }
            p.C[(long)row * p.ldc + oc] = v;
          }
        }
      }
    }
  } else
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = n0 + wn * (32 * NT) + j * 32 + l31;
    const bool col_ok = col < p.N;
    const float bv = (p.bias != nullptr && col_ok) ? p.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int rbase = m0 + wm * (32 * MT) + i * 32 + 4 * lh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rbase + (r & 3) + 8 * (r >> 2);
        if (col_ok && row < p.M) {
          float* c = p.C + (long)row * p.ldc + col;
          float v = acc[i][j][r] + bv;
          if constexpr (ACC != 0) v += *c;
          *c = v;
        }
      }
    }
  }
  if constexpr (DBG == 3) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wg_stamp(3);
  }
}

template <int MT, int NT, int NST, int EPI = EPI_PLAIN, int ACC = 0, int SEQ = 0, int DBG = 0, int PIN = 0, int PIPE = 0>
static int launch_gemm_x6(GemmX6Params p, hipStream_t st) {
  constexpr int BM = 64 * MT, BN = 64 * NT;
  constexpr size_t smem = (size_t)NST * (6 * BM + 6 * BN) * 16;
  static_assert(smem <= 160 * 1024, "LDS stages of this tile shape");
  p.m_tiles = ceil_div(p.M, BM);
  p.n_tiles = ceil_div(p.N, BN);
  IX_ARG((long)p.n_tiles * BN <= p.Npad, "gemm_x6: packed weights padded to %d features, the %d-wide tile needs %d", p.Npad, BN, p.n_tiles * BN);
  if constexpr (PIPE != 0) IX_ARG(p.K > 0 && p.K % 64 == 0, "gemm_x6: the pipelined loop takes its steps in fours, K %d", p.K);
  const int taps = (p.K >> 4) / p.tap_steps;  // the last tap reads taps - 1 rows below the tile
  IX_ARG(p.arow0 + (long)p.m_tiles * BM + taps - 1 <= p.Mpad, "gemm_x6: activation planes hold %ld rows, the %d-row tiles reach row %ld", p.Mpad, BM,
         p.arow0 + (long)p.m_tiles * BM + taps - 1);
  auto kern = gemm_x6_kernel<MT, NT, NST, EPI, ACC, SEQ, DBG, PIN, PIPE>;
  static bool done = false;
  if (!done) {
    IX_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    done = true;
  }
  hipLaunchKernelGGL(kern, dim3(p.m_tiles * p.n_tiles), dim3(256), smem, st, p);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

// the kernel instantiation for what the tile writes (p.epi, p.accumulate, p.gate_seq_off); PAIR: this tile shape takes the pair epilogues
template <int MT, int NT, int NST, bool PAIR, int PIPE = 0>
static int launch_gemm_x6_epilogue(const GemmX6Params& p, hipStream_t st) {
  if (p.epi == EPI_PLAIN)
    return p.accumulate ? launch_gemm_x6<MT, NT, NST, EPI_PLAIN, 1, 0, 0, 0, PIPE>(p, st) : launch_gemm_x6<MT, NT, NST, EPI_PLAIN, 0, 0, 0, 0, PIPE>(p, st);
  if constexpr (PAIR) {
    if (p.epi == EPI_SWIGLU) return launch_gemm_x6<MT, NT, NST, EPI_SWIGLU, 0, 0, 0, 0, PIPE>(p, st);
    if (p.epi == EPI_GATE)
      return p.gate_seq_off ? launch_gemm_x6<MT, NT, NST, EPI_GATE, 0, 1, 0, 0, PIPE>(p, st) : launch_gemm_x6<MT, NT, NST, EPI_GATE, 0, 0, 0, 0, PIPE>(p, st);
  }
  set_error("gemm_x6: epilogue %d on a tile shape built without it", p.epi);
  return IXTTS_ERR_ARG;
}

}  // namespace ixtts

using namespace ixtts;

extern "C" size_t ixtts_gemm_x6_packed_bytes(int N, int K) {
  if (N <= 0 || K <= 0 || K % 64) return 0;
  const size_t Npad = (size_t)(N + 255) / 256 * 256;
  return (size_t)(K / 16) * 6 * Npad * 16;
}

extern "C" int ixtts_gemm_x6_pack(const float* w_dev, void* packed_dev, int N, int K, void* stream) {
  IX_ARG(w_dev && packed_dev && N > 0 && K > 0 && K % 64 == 0, "gemm_x6_pack: bad argument (K must be a multiple of 64)");
  const int Npad = (N + 255) / 256 * 256;
  const long total = (long)(K / 8) * Npad;
  hipLaunchKernelGGL(gemm_x6_pack_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, w_dev,
                     reinterpret_cast<uint4*>(packed_dev), N, K, Npad);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

extern "C" long ixtts_gemm_x6_rows_padded(long rows) { return rows <= 0 ? 0 : (rows + 255) / 256 * 256 + 256; }

extern "C" int ixtts_gemm_x6_split(const float* a_dev, long lda, void* planes_dev, long rows, int K, void* stream) {
  IX_ARG(a_dev && planes_dev && rows > 0 && K > 0 && K % 64 == 0, "gemm_x6_split: bad argument (K must be a multiple of 64)");
  IX_ARG(lda >= K && lda % 4 == 0 && (reinterpret_cast<uintptr_t>(a_dev) & 15) == 0, "gemm_x6_split: rows must be 16-byte aligned (lda %ld)", lda);
  const long Mpad = ixtts_gemm_x6_rows_padded(rows);
  hipLaunchKernelGGL(gemm_x6_split_kernel<0>, dim3((unsigned)(Mpad / 64), K / 64), dim3(256), 0, (hipStream_t)stream, a_dev, lda,
                     reinterpret_cast<uint4*>(planes_dev), (int)rows, K, Mpad);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

extern "C" int ixtts_gemm_x6_split_halo(const float* a_dev, long lda, void* planes_dev, long rows, int K, int T, int left, int right, void* stream) {
  IX_ARG(a_dev && planes_dev && rows > 0 && K > 0 && K % 64 == 0, "gemm_x6_split_halo: bad argument (K must be a multiple of 64)");
  IX_ARG(lda >= K && lda % 4 == 0 && (reinterpret_cast<uintptr_t>(a_dev) & 15) == 0, "gemm_x6_split_halo: rows must be 16-byte aligned (lda %ld)", lda);
  IX_ARG(left >= 0 && right >= 0 && T > left && T > right && rows % (left + T + right) == 0,
         "gemm_x6_split_halo: bad shape rows=%ld T=%d left=%d right=%d (rows = whole sequences of left + T + right)", rows, T, left, right);
  const long Mpad = ixtts_gemm_x6_rows_padded(rows);
  hipLaunchKernelGGL(gemm_x6_split_kernel<1>, dim3((unsigned)(Mpad / 64), K / 64), dim3(256), 0, (hipStream_t)stream, a_dev, lda,
                     reinterpret_cast<uint4*>(planes_dev), (int)rows, K, Mpad, T, left, right);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

extern "C" int ixtts_gemm_x6_split_halo_varlen(const float* a_dev, long lda, void* planes_dev, long rows, int K, const int* seq_off_dev, int nseq, int left,
                                               int right, void* stream) {
  IX_ARG(a_dev && planes_dev && seq_off_dev && rows > 0 && K > 0 && K % 64 == 0, "gemm_x6_split_halo_varlen: bad argument (K must be a multiple of 64)");
  IX_ARG(lda >= K && lda % 4 == 0 && (reinterpret_cast<uintptr_t>(a_dev) & 15) == 0, "gemm_x6_split_halo_varlen: rows must be 16-byte aligned (lda %ld)", lda);
  IX_ARG(nseq > 0 && left >= 0 && right >= 0, "gemm_x6_split_halo_varlen: bad shape nseq=%d left=%d right=%d", nseq, left, right);
  const long Mpad = ixtts_gemm_x6_rows_padded(rows);
  hipLaunchKernelGGL(gemm_x6_split_kernel<2>, dim3((unsigned)(Mpad / 64), K / 64), dim3(256), 0, (hipStream_t)stream, a_dev, lda,
                     reinterpret_cast<uint4*>(planes_dev), (int)rows, K, Mpad, 0, left, right, seq_off_dev, nseq);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

static long device_cu_count() {  // of the current device, asked once
  static const long n = [] {
    int dev = 0, cus = 0;
    return (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) ? (long)cus : 0L;
  }();
  return n;
}

static int run_gemm_x6(GemmX6Params p, int tile, hipStream_t st) {
  if (tile == 0) {  // by fill of the 256 CUs: the wider tile while it still gives most CUs work (operand bytes per MFMA fall with the tile)
    const long t42 = (long)ceil_div(p.M, 256) * ceil_div(p.N, 128);
    tile = t42 >= 140 ? 2 : 3;
    // no more 128 x 128 tiles than CUs: tile 3's two workgroups per CU never meet, each SIMD holds one wave and nothing hides its
    // issue cycles -- the pipelined loop hides them itself.  IXTTS_GEMM_X6_PIPE=0: tile 3 there as before (A/B runs, tests).
    static const bool pipe = !(getenv("IXTTS_GEMM_X6_PIPE") && !strcmp(getenv("IXTTS_GEMM_X6_PIPE"), "0"));
    if (tile == 3 && pipe && (long)ceil_div(p.M, 128) * ceil_div(p.N, 128) <= device_cu_count()) tile = 6;
  }
  switch (tile) {
    // two workgroups per CU (2 x 73.7 KB of LDS): one's copies, fragment reads and epilogue run under the other's MFMAs
    case 2: return launch_gemm_x6_epilogue<4, 2, 2, true>(p, st);
    case 3: return launch_gemm_x6_epilogue<2, 2, 3, true>(p, st);
    // one workgroup per CU, copies three steps ahead (A/B timing; plain epilogue only)
    case 4: return launch_gemm_x6_epilogue<4, 2, 4, false>(p, st);
    case 5: return launch_gemm_x6_epilogue<2, 2, 4, false>(p, st);
    // one workgroup per CU, pipelined loop: next step's fragment reads and the copies issued among the MFMAs
    case 6: return launch_gemm_x6_epilogue<2, 2, 4, true, 1>(p, st);
  }
  if (tile >= 12 && (p.epi != EPI_PLAIN || p.accumulate)) {
    set_error("gemm_x6: the developer variants (tile %d) are built with the plain, overwriting epilogue only", tile);
    return IXTTS_ERR_ARG;
  }
  switch (tile) {
    // developer timing variants (results meaningless)
    case 12: return launch_gemm_x6<4, 2, 2, EPI_PLAIN, 0, 0, 1>(p, st);
    case 22: return launch_gemm_x6<4, 2, 2, EPI_PLAIN, 0, 0, 2>(p, st);
    case 32: return launch_gemm_x6<4, 2, 2, EPI_PLAIN, 0, 0, 3>(p, st);
    case 33: return launch_gemm_x6<2, 2, 3, EPI_PLAIN, 0, 0, 3>(p, st);
    case 36: return launch_gemm_x6<2, 2, 4, EPI_PLAIN, 0, 0, 3, 0, 1>(p, st);
    // the loop with a fence between a step's MFMAs and its closing wait (results as tiles 2 / 3; A/B timing of the fence)
    case 42: return launch_gemm_x6<4, 2, 2, EPI_PLAIN, 0, 0, 0, 1>(p, st);
    case 43: return launch_gemm_x6<2, 2, 3, EPI_PLAIN, 0, 0, 0, 1>(p, st);
  }
  set_error("gemm_x6: tile %d (0 auto; 2 / 3: 256x128 / 128x128, two workgroups per CU; 4 / 5: the same, one per CU with a 4-stage ring; 6: 128x128, one per CU, pipelined loop)", tile);
  return IXTTS_ERR_ARG;
}

extern "C" int ixtts_gemm_x6_f32(const void* a_planes_dev, long rows_total, long row0, const void* packed_dev, const float* bias_dev, float* c_dev,
                                 long ldc, int M, int N, int K, int accumulate, int tile, void* stream) {
  IX_ARG(a_planes_dev && packed_dev && c_dev && M > 0 && N > 0 && K > 0 && K % 64 == 0, "gemm_x6: bad argument (K must be a multiple of 64: the split pass works on 64-wide k blocks)");
  IX_ARG(ldc >= N && row0 >= 0 && row0 + M <= rows_total, "gemm_x6: rows [%ld, %ld) of %ld, ldc %ld", row0, row0 + M, rows_total, ldc);
  GemmX6Params p;
  p.Ap = reinterpret_cast<const uint4*>(a_planes_dev); p.Mpad = ixtts_gemm_x6_rows_padded(rows_total); p.arow0 = row0;
  p.Wp = reinterpret_cast<const uint4*>(packed_dev); p.bias = bias_dev; p.C = c_dev; p.ldc = ldc;
  p.M = M; p.N = N; p.Npad = (N + 255) / 256 * 256; p.K = K; p.accumulate = accumulate ? 1 : 0; p.m_tiles = p.n_tiles = 0;
  p.tap_steps = K >> 4; p.epi = EPI_PLAIN; p.gate = nullptr; p.gate_ld = 0; p.rows_per_batch = 1; p.nbatch = 1; p.gate_seq_off = nullptr;
  p.dbg = (tile == 32 || tile == 33 || tile == 36) ? reinterpret_cast<unsigned long long*>(const_cast<float*>(bias_dev)) : nullptr;  // developer stamps travel in the bias slot
  if (p.dbg) p.bias = nullptr;
  return run_gemm_x6(p, tile, (hipStream_t)stream);
}

extern "C" int ixtts_gemm_x6_pair_f32(const void* a_planes_dev, long rows_total, long row0, int taps, const void* packed_dev, const float* bias_dev,
                                      const float* gate_dev, long gate_ld, long rows_per_batch, int nbatch, float* c_dev, long ldc, int M, int N, int K,
                                      int epilogue, int tile, void* stream) {
  IX_ARG(a_planes_dev && packed_dev && c_dev && M > 0 && N > 0 && taps > 0 && K > 0, "gemm_x6_pair: bad argument");
  IX_ARG(K % taps == 0 && (K / taps) % 64 == 0 && N % 64 == 0, "gemm_x6_pair: K %d = %d taps of a multiple of 64, N %d a multiple of 64", K, taps, N);
  IX_ARG(epilogue == EPI_SWIGLU || (epilogue == EPI_GATE && gate_dev && rows_per_batch > 0 && nbatch > 0 && gate_ld >= N / 2),
         "gemm_x6_pair: epilogue %d (1 swiglu; 2 gate, with gate biases)", epilogue);
  IX_ARG(ldc >= N / 2 && row0 >= 0 && row0 + M + taps - 1 <= rows_total, "gemm_x6_pair: rows [%ld, %ld) + %d taps of %ld, ldc %ld", row0, row0 + M, taps,
         rows_total, ldc);
  IX_ARG(tile == 0 || tile == 2 || tile == 3 || tile == 6, "gemm_x6_pair: tile %d (0 auto, 2, 3, 6)", tile);
  GemmX6Params p;
  p.Ap = reinterpret_cast<const uint4*>(a_planes_dev); p.Mpad = ixtts_gemm_x6_rows_padded(rows_total); p.arow0 = row0;
  p.Wp = reinterpret_cast<const uint4*>(packed_dev); p.bias = bias_dev; p.C = c_dev; p.ldc = ldc;
  p.M = M; p.N = N; p.Npad = (N + 255) / 256 * 256; p.K = K; p.accumulate = 0; p.m_tiles = p.n_tiles = 0;
  p.tap_steps = (K / taps) >> 4; p.epi = epilogue; p.gate = gate_dev; p.gate_ld = gate_ld; p.rows_per_batch = rows_per_batch; p.nbatch = nbatch;
  p.gate_seq_off = nullptr;
  p.dbg = nullptr;
  return run_gemm_x6(p, tile, (hipStream_t)stream);
}

extern "C" int ixtts_gemm_x6_pair_gate_varlen_f32(const void* a_planes_dev, long rows_total, long row0, int taps, const void* packed_dev, const float* bias_dev,
                                                  const float* gate_dev, long gate_ld, const int* seq_off_dev, int nseq, float* c_dev, long ldc, int M, int N,
                                                  int K, int tile, void* stream) {
  IX_ARG(seq_off_dev && nseq > 0, "gemm_x6_pair_gate_varlen: null offsets table or nseq %d", nseq);
  IX_ARG(a_planes_dev && packed_dev && c_dev && gate_dev && M > 0 && N > 0 && taps > 0 && K > 0 && gate_ld >= N / 2, "gemm_x6_pair_gate_varlen: bad argument");
  IX_ARG(K % taps == 0 && (K / taps) % 64 == 0 && N % 64 == 0, "gemm_x6_pair_gate_varlen: K %d = %d taps of a multiple of 64, N %d a multiple of 64", K, taps, N);
  IX_ARG(ldc >= N / 2 && row0 >= 0 && row0 + M + taps - 1 <= rows_total, "gemm_x6_pair_gate_varlen: rows [%ld, %ld) + %d taps of %ld, ldc %ld", row0, row0 + M,
         taps, rows_total, ldc);
  IX_ARG(tile == 0 || tile == 2 || tile == 3 || tile == 6, "gemm_x6_pair_gate_varlen: tile %d (0 auto, 2, 3, 6)", tile);
  GemmX6Params p;
  p.Ap = reinterpret_cast<const uint4*>(a_planes_dev); p.Mpad = ixtts_gemm_x6_rows_padded(rows_total); p.arow0 = row0;
  p.Wp = reinterpret_cast<const uint4*>(packed_dev); p.bias = bias_dev; p.C = c_dev; p.ldc = ldc;
  p.M = M; p.N = N; p.Npad = (N + 255) / 256 * 256; p.K = K; p.accumulate = 0; p.m_tiles = p.n_tiles = 0;
  p.tap_steps = (K / taps) >> 4; p.epi = EPI_GATE; p.gate = gate_dev; p.gate_ld = gate_ld; p.rows_per_batch = 1; p.nbatch = nseq;
  p.gate_seq_off = seq_off_dev;
  p.dbg = nullptr;
  return run_gemm_x6(p, tile, (hipStream_t)stream);
}
