// gpt_rows.hip -- batched ("rows") causal pass of the GPT-2 trunk on gfx950: prefill of the
// prompt (row G1, model_v2.py:144-155) and the latent forward (row G9, model_v2.py:554-596).
//
// T rows go through the 24 layers together: LayerNorm rows -> MFMA GEMM against the same
// transposed/folded weight arena the decode GEMVs stream (QKV with KV-cache scatter, out-proj
// + residual, FC + gelu_new, MLP-out + residual) and a causal row-attention that reads the
// cache.  fp32 mode uses v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chains, parity mode); in the bf16
// and fp16 modes the producers (LayerNorm, attention, gelu) write rows of the weights' type and the
// GEMMs run on v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x16_f16 with fp32 accumulation (fp16 rows
// saturate at +-65504 where they are written).
//
// Reference arithmetic: indextts/gpt/transformers_gpt2.py:480-667.
#include "gpt_engine.h"
#include "gpt_kernels.h"

namespace ixtts {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// the 32x32x16 MFMA of a 16-bit element type (bf16 | fp16), fp32 accumulation
template <typename ET>
struct RowsEl;
template <>
struct RowsEl<bf16> {
  typedef bf16x8 vec8;
  __device__ static __forceinline__ f32x16 mfma(const vec8& a, const vec8& b, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <>
struct RowsEl<f16> {
  typedef f16x8 vec8;
  __device__ static __forceinline__ f32x16 mfma(const vec8& a, const vec8& b, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// two fp32 -> packed bf16 pair (round-to-nearest-even, the plain cast lowers to v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned int pack_bf16x2(float a, float b) {
  const unsigned short lo = __builtin_bit_cast(unsigned short, (__bf16)a);
  const unsigned short hi = __builtin_bit_cast(unsigned short, (__bf16)b);
  return (unsigned int)lo | ((unsigned int)hi << 16);
}

// ---- (x - mean) * rstd per row (gain/bias are folded into the next matrix); one wave per row
template <int K, typename OT = float>
__global__ __launch_bounds__(256) void ln_rows_kernel(const float* __restrict__ x, OT* __restrict__ y, int T) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= T) return;
  constexpr int PL = K / 64;  // elements per lane (20 for 1280, 2 for 128)
  const float* xr = x + (size_t)row * K;
  float v[PL];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    v[i] = xr[lane + 64 * i];
    s += v[i];
  }
  const float mean = wave_sum(s) * (1.0f / K);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    const float d = v[i] - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / K) + 1e-5f);
  OT* yr = y + (size_t)row * K;
#pragma unroll
  for (int i = 0; i < PL; ++i) store_kv(yr + lane + 64 * i, (v[i] - mean) * rstd);
}

// ---- ln_f (explicit affine) then final_norm (explicit affine) per row -> latent rows.  One wave per row; the row's arithmetic is
// final_norm_row, shared by the one-sequence kernel and the scatter of a packed latent pass (latent_norm_scatter_kernel)
template <int K>
__device__ __forceinline__ void final_norm_row(const float* __restrict__ x, float* __restrict__ y, const size_t row_in, const size_t row_out, const int lane,
                                               const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                               const float* __restrict__ b2) {
  constexpr int PL = K / 64;
  const float* xr = x + row_in * K;
  float v[PL];
#pragma unroll
  for (int i = 0; i < PL; ++i) v[i] = xr[lane + 64 * i];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const float* w = pass == 0 ? w1 : w2;
    const float* b = pass == 0 ? b1 : b2;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PL; ++i) s += v[i];
    const float mean = wave_sum(s) * (1.0f / K);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PL; ++i) {
      const float d = v[i] - mean;
      q = fmaf(d, d, q);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / K) + 1e-5f);
#pragma unroll
    for (int i = 0; i < PL; ++i) v[i] = (v[i] - mean) * rstd * w[lane + 64 * i] + b[lane + 64 * i];
  }
  float* yr = y + row_out * K;
#pragma unroll
  for (int i = 0; i < PL; ++i) yr[lane + 64 * i] = v[i];
}
template <int K>
__global__ __launch_bounds__(256) void final_norm_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int T,
                                                               const float* __restrict__ w1, const float* __restrict__ b1,
                                                               const float* __restrict__ w2, const float* __restrict__ b2) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= T) return;
  final_norm_row<K>(x, y, (size_t)row, (size_t)row, lane, w1, b1, w2, b2);
}

// ---- GEMM: C[T][N] = A[T][K] . Wt[N][K]^T + bias
enum { RE_QKV = 0, RE_RESID = 1, RE_GELU = 2, RE_QKV_PACKED = 3 };

struct GemmArgs {
  const float* A;    // [T][K] fp32
  const void* wt;    // [N][K]
  const float* bias; // [N]
  float* out;        // RE_QKV: q [T][D]; RE_RESID: x [T][N] (+=); RE_GELU: ff [T][N]
  void* kcache;      // RE_QKV: slot+layer base [H][smax][64]
  void* vcache;
  int T, N, K, pos0, smax, D;
};

// RE_QKV_PACKED (ixtts_gpt_prefill_many): the T rows are the valid rows of several sequences one after the other; kcache / vcache
// are the LAYER's bases and row m's K/V go to cache row row_at[m] = slot * H * smax + position (counted in rows of HD elements
// from that base, head 0) -- the one line in which the epilogue differs from RE_QKV
struct GemmArgsPacked : GemmArgs {
  const int* row_at;  // [T]
};

constexpr int GBN = 128;

// Tile BM x 128 x BK, 4 waves as 2 x 2, wave tile (BM/2) x 64.  bf16: BK = 64, both operands staged as bf16 in LDS (the
// fp32 activations are converted in the staging pass), rows padded to 144 B so the 16-byte fragment reads of 8 consecutive
// rows fall in 8 different bank groups; fp32: BK = 32, pitch 33.  The global loads of k-tile i+1 are issued before the
// MFMAs of k-tile i and written to LDS after them (one register set, one LDS buffer, two barriers per k-tile).
template <typename WT, int EPI, typename KVT, int BM, typename GA = GemmArgs>
__global__ __launch_bounds__(256) void gemm_rows_kernel(GA g) {
  constexpr bool F32 = sizeof(WT) == 4;
  constexpr int BK = F32 ? 32 : 64;
  constexpr int MI = BM / 64;                              // 32-row blocks per wave
  constexpr int PITCH = F32 ? (BK + 1) : (BK + 8) / 2;     // floats per LDS row (bf16: 72 halfs = 36 floats)
  __shared__ __attribute__((aligned(16))) float As[BM * PITCH];
  __shared__ __attribute__((aligned(16))) float Ws[GBN * PITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * GBN;

  f32x16 acc[MI][2];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][j][r] = 0.f;

  constexpr int NA = BM * BK / 4 / 256;                    // float4 of A per thread per k-tile
  constexpr int NW = F32 ? GBN * BK / 4 / 256 : GBN * BK / 8 / 256;  // 16-byte pieces of W per thread
  constexpr int AC = BK / 4;                               // float4 per A row
  constexpr int WC = F32 ? BK / 4 : BK / 8;                // 16-byte pieces per W row
  constexpr int PD = 1;  // k-tiles in flight ahead of the MFMAs (register sets); r01: 3 sets measured slower (latent pass 21.4 vs 16.6 ms)
  float4 aR[PD][NA];
  uint4 wR[PD][NW];
  // (loads are unconditional -- rows and k offsets clamped -- so the compiler's vmcnt counting stays exact: a stage is
  //  written to LDS as soon as ITS loads have landed, with the younger stages still in flight)
  auto stage_load = [&](float4 (&ar)[NA], uint4 (&wr)[NW], int k0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = tid + i * 256;
      const int row = min(m0 + idx / AC, g.T - 1);  // rows beyond T repeat the last one; their outputs are never stored
      ar[i] = *reinterpret_cast<const float4*>(g.A + (size_t)row * g.K + k0 + (idx % AC) * 4);
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int idx = tid + i * 256;
      const int row = min(n0 + idx / WC, g.N - 1);
      wr[i] = *reinterpret_cast<const uint4*>(reinterpret_cast<const WT*>(g.wt) + (size_t)row * g.K + k0 + (idx % WC) * (16 / (int)sizeof(WT)));
    }
  };
  auto stage_write = [&](const float4 (&ar)[NA], const uint4 (&wr)[NW]) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = tid + i * 256;
      const int row = idx / AC, c4 = idx % AC;
      if constexpr (F32) {
        float* d = As + row * PITCH + c4 * 4;
        d[0] = ar[i].x; d[1] = ar[i].y; d[2] = ar[i].z; d[3] = ar[i].w;
      } else {
        uint2 pk;
        pk.x = pack_bf16x2(ar[i].x, ar[i].y);
        pk.y = pack_bf16x2(ar[i].z, ar[i].w);
        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(As) + row * (PITCH * 2) + c4 * 4) = pk;
      }
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int idx = tid + i * 256;
      const int row = idx / WC, c = idx % WC;
      if constexpr (F32) {
        float* d = Ws + row * PITCH + c * 4;
        d[0] = __uint_as_float(wr[i].x); d[1] = __uint_as_float(wr[i].y); d[2] = __uint_as_float(wr[i].z); d[3] = __uint_as_float(wr[i].w);
      } else {
        *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(Ws) + row * (PITCH * 2) + c * 8) = wr[i];
      }
    }
  };

  const int nkt = g.K / BK;
#pragma unroll
  for (int s = 0; s < PD; ++s) stage_load(aR[s], wR[s], min(s, nkt - 1) * BK);
  for (int kt0 = 0; kt0 < nkt; kt0 += PD) {
#pragma unroll
    for (int s = 0; s < PD; ++s) {
      if (kt0 + s >= nkt) break;
      __syncthreads();  // every wave is done with the previous k-tile
      stage_write(aR[s], wR[s]);
      __syncthreads();
      stage_load(aR[s], wR[s], min(kt0 + s + PD, nkt - 1) * BK);
    if constexpr (F32) {
#pragma unroll
      for (int kk = 0; kk < BK; kk += 2) {
        float a[MI], b[2];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) a[mi] = As[(wm * (BM / 2) + mi * 32 + l31) * PITCH + kk + lh];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = Ws[(wn * 64 + j * 32 + l31) * PITCH + kk + lh];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[mi][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], b[j], acc[mi][j], 0, 0, 0);
      }
    } else {
      const unsigned short* A16 = reinterpret_cast<const unsigned short*>(As);
      const unsigned short* W16 = reinterpret_cast<const unsigned short*>(Ws);
#pragma unroll
      for (int kk = 0; kk < BK; kk += 16) {
        bf16x8 a[MI], b[2];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) a[mi] = *reinterpret_cast<const bf16x8*>(A16 + (wm * (BM / 2) + mi * 32 + l31) * (PITCH * 2) + kk + lh * 8);
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const bf16x8*>(W16 + (wn * 64 + j * 32 + l31) * (PITCH * 2) + kk + lh * 8);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[mi][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[j], acc[mi][j], 0, 0, 0);
      }
    }
    }
  }
  // ---- epilogue (C layout: col = lane&31 -> n, row = (r&3) + 8*(r>>2) + 4*(lane>>5) -> m)
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + l31;
      if (n >= g.N) continue;
      const float bias = g.bias[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * (BM / 2) + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m >= g.T) continue;
        const float v = acc[mi][j][r] + bias;
        if constexpr (EPI == RE_RESID) {
          float* o = g.out + (size_t)m * g.N + n;
          *o = *o + v;
        } else if constexpr (EPI == RE_GELU) {
          g.out[(size_t)m * g.N + n] = gelu_new_f(v);
        } else if constexpr (EPI == RE_QKV_PACKED) {
          if (n < g.D) {
            g.out[(size_t)m * g.D + n] = v;
          } else {
            const int which = n / g.D;
            const int c = n - which * g.D;
            const int hh = c / HD, d = c % HD;
            KVT* cache = reinterpret_cast<KVT*>(which == 1 ? g.kcache : g.vcache);
            store_kv(cache + ((size_t)hh * g.smax + g.row_at[m]) * HD + d, v);
          }
        } else {
          if (n < g.D) {
            g.out[(size_t)m * g.D + n] = v;
          } else {
            const int which = n / g.D;
            const int c = n - which * g.D;
            const int hh = c / HD, d = c % HD;
            KVT* cache = reinterpret_cast<KVT*>(which == 1 ? g.kcache : g.vcache);
            store_kv(cache + ((size_t)hh * g.smax + g.pos0 + m) * HD + d, v);
          }
        }
      }
    }
}

// ---- 16-bit GEMM of the rows path (ET = bf16 | f16; written for bf16, fp16 swaps the MFMA and the stores): C[T][N] = A16[T][K] . Wt[N][K]^T (+ epilogue), tile 128 x 128 x 64, 4 waves (2 x 2),
// wave tile 64 x 64 on v_mfma_f32_32x32x16_bf16.  Both operands are bf16 in global memory (the LayerNorm / attention /
// gelu producers write bf16 rows), so a k-tile is 32 one-KiB pieces copied global -> LDS by LDS-DMA
// (global_load_lds_dwordx4: no VGPRs, no ds_write pass) into two LDS buffers: the copy of k-tile i+1 is in flight under the
// MFMAs of k-tile i (raw s_barrier + counted vmcnt: a __syncthreads would drain it).  (A ring of 4 buffers measured the
// same: the copies are not what bounds the loop.)  The LDS image is row-linear (what
// the DMA writes); the 16-byte granule g of row r sits at position g ^ ((r >> 1) & 7) -- swizzled on the SOURCE address
// and on the fragment read.  A ds_read_b128 is served in 4 groups of 16 lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31}, +32)
// over 64 banks = 16 granules: with 128-byte rows the granule slot is 8 (r & 1) + position, and (r >> 1) & 7 takes 8
// different values over each group's even rows and over its odd rows -> conflict-free (g ^ (r & 7) was 2-way: PMC).
struct GemmArgs16 {
  const unsigned short* A;  // [T][K] bf16
  const unsigned short* wt; // [N][K] bf16
  const float* bias;        // [N]
  void* out;                // RE_QKV: q fp32 [T][D]; RE_RESID: x fp32 [T][N] (+=); RE_GELU: ff bf16 [T][N]
  void* kcache;             // RE_QKV: slot+layer base [H][smax][64]
  void* vcache;
  int T, N, K, pos0, smax, D;
};

struct GemmArgs16Packed : GemmArgs16 {  // RE_QKV_PACKED, as GemmArgsPacked
  const int* row_at;  // [T]
};

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

constexpr int G16_NBUF = 2;                       // LDS buffers: NBUF - 1 k-tiles of copies in flight under the MFMAs
constexpr int G16_TILE = 128 * 64 * 2;            // 16 KiB per operand tile
constexpr int G16_SMEM = G16_NBUF * 2 * G16_TILE; // 64 KiB: two workgroups per CU

template <int EPI, typename KVT, typename GA = GemmArgs16>
__global__ __launch_bounds__(256) void gemm_rows_bf16_kernel(GA g) {  // KVT is also the operands' element type
  using EL = RowsEl<KVT>;
  typedef typename EL::vec8 vec8;
  constexpr int BM = 128, BN = 128, BK = 64, TILE = G16_TILE, NBUF = G16_NBUF;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_raw[];
  unsigned char (*smem)[2][TILE] = reinterpret_cast<unsigned char (*)[2][TILE]>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][j][r] = 0.f;

  // this wave's 4 + 4 DMA pieces of a k-tile: piece c covers rows 8c .. 8c+7, lane -> (row, swizzled granule)
  const unsigned short* asrc[4];
  const unsigned short* wsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 8 + (lane >> 3);
    const int gran = (lane & 7) ^ ((row >> 1) & 7);
    asrc[i] = g.A + (size_t)min(m0 + row, g.T - 1) * g.K + gran * 8;  // rows beyond T repeat the last one; never stored
    wsrc[i] = g.wt + (size_t)min(n0 + row, g.N - 1) * g.K + gran * 8;
  }
  auto issue = [&](int kt, int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      glds16(asrc[i] + kt * BK, &smem[buf][0][(wave * 4 + i) * 1024]);
      glds16(wsrc[i] + kt * BK, &smem[buf][1][(wave * 4 + i) * 1024]);
    }
  };
  const int nkt = g.K / BK;
#pragma unroll
  for (int p = 0; p < NBUF - 1; ++p) issue(min(p, nkt - 1), p);
  for (int kt = 0; kt < nkt; ++kt) {
    // (past the end the last tile is re-copied into an idle buffer: keeps the outstanding count fixed)
    issue(min(kt + NBUF - 1, nkt - 1), (kt + NBUF - 1) % NBUF);
    static_assert(NBUF == 2, "the immediate below is 8 * (NBUF - 1)");
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // everything but the youngest k-tile (8 pieces) has landed
    __builtin_amdgcn_s_barrier();
    const unsigned char* At = smem[kt % NBUF][0];
    const unsigned char* Wt = smem[kt % NBUF][1];
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      vec8 a[2], b[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int row = wm * 64 + mi * 32 + l31;
        a[mi] = *reinterpret_cast<const vec8*>(At + row * 128 + (((kk * 2 + lh) ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = wn * 64 + j * 32 + l31;
        b[j] = *reinterpret_cast<const vec8*>(Wt + row * 128 + (((kk * 2 + lh) ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[mi][j] = EL::mfma(a[mi], b[j], acc[mi][j]);
    }
    __builtin_amdgcn_s_barrier();  // every wave is done with this buffer before the next iteration's copy lands in it
  }
  // ---- epilogue (C layout: col = lane&31 -> n, row = (r&3) + 8*(r>>2) + 4*(lane>>5) -> m).  Loads first, all of them,
  // unconditionally (indices clamped): a residual load under the row-bound branch was waited for on the spot, 64 dependent
  // round trips per lane (~25 us per launch whatever the GEMM size).  Only the stores are predicated.
  float bias[2];
  int ncol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    ncol[j] = n0 + wn * 64 + j * 32 + l31;
    bias[j] = g.bias[min(ncol[j], g.N - 1)];
  }
  if constexpr (EPI == RE_RESID) {
    float* xo = reinterpret_cast<float*>(g.out);
    float old[2][2][16];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = min(m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, g.T - 1);
          old[mi][j][r] = xo[(size_t)m * g.N + min(ncol[j], g.N - 1)];
        }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (m < g.T && ncol[j] < g.N) xo[(size_t)m * g.N + ncol[j]] = old[mi][j][r] + (acc[mi][j][r] + bias[j]);
        }
  } else if constexpr (EPI == RE_QKV_PACKED) {
    // the rows' cache positions first, all of them, not under the row bound (clamped): the same rule as the residual loads above.
    // Only a workgroup whose column tile holds K or V columns needs them (workgroup-uniform: a tile of Q columns skips the loads)
    int at[2][16] = {};
    if (n0 + BN > g.D) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) at[mi][r] = g.row_at[min(m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, g.T - 1)];
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = ncol[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (m >= g.T || n >= g.N) continue;
          const float v = acc[mi][j][r] + bias[j];
          if (n < g.D) {
            reinterpret_cast<float*>(g.out)[(size_t)m * g.D + n] = v;
          } else {
            const int which = n / g.D;
            const int c = n - which * g.D;
            const int hh = c / HD, d = c % HD;
            KVT* cache = reinterpret_cast<KVT*>(which == 1 ? g.kcache : g.vcache);
            store_kv(cache + ((size_t)hh * g.smax + at[mi][r]) * HD + d, v);
          }
        }
      }
  } else {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = ncol[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (m >= g.T || n >= g.N) continue;
          const float v = acc[mi][j][r] + bias[j];
          if constexpr (EPI == RE_GELU) {
            // gelu_new(v) = v * sigmoid(2u), u = sqrt(2/pi) (v + 0.044715 v^3): one exp instead of tanhf (the result is rounded to bf16)
            const float u2 = 1.5957691216057308f * (v + 0.044715f * v * v * v);
            store_kv(reinterpret_cast<KVT*>(g.out) + (size_t)m * g.N + n, v / (1.0f + __expf(-u2)));
          } else {
            if (n < g.D) {
              reinterpret_cast<float*>(g.out)[(size_t)m * g.D + n] = v;
            } else {
              const int which = n / g.D;
              const int c = n - which * g.D;
              const int hh = c / HD, d = c % HD;
              KVT* cache = reinterpret_cast<KVT*>(which == 1 ? g.kcache : g.vcache);
              store_kv(cache + ((size_t)hh * g.smax + g.pos0 + m) * HD + d, v);
            }
          }
        }
      }
  }
}

// ---- causal attention over rows: grid (H, T); row t attends keys [valid_from, pos0 + t]
struct AttnRowsArgs {
  const float* q;      // [T][D]
  const void* kcache;  // slot+layer base [H][smax][64]
  const void* vcache;
  void* out;           // [T][D], fp32 or bf16 (OT)
  int T, D, smax, pos0, valid_from;
};

// (the statements are attn_rows_body.h, shared as text with the two packed row kernels below)
template <typename KVT, typename OT = float>
__global__ __launch_bounds__(256) void attn_rows_kernel(AttnRowsArgs a) {
#define ROWS_ROW ((int)blockIdx.y)
#define ROWS_K0 0
#include "attn_rows_body.h"
#undef ROWS_ROW
#undef ROWS_K0
}

// The packed pass of ixtts_gpt_prefill_many: several sequences' rows one after the other in q / out, each sequence with its own
// slot cache, T, pos0 and valid_from.  A workgroup of the attention kernels below serves ONE sequence: it builds that sequence's
// AttnRowsArgs from the table and runs on it the one-sequence kernel's statements (attn_rows_body.h, attn_rows_flash_body.h): query
// partition, key-tile origin, wave skips, masks and clamps are those of the solo launch.
struct AttnPackedArgs {
  const float* q;         // [sum T][D]
  const void* kcache;     // LAYER base [slot][H][smax][64]
  const void* vcache;
  void* out;              // [sum T][D]
  const PackSeq* seqs;
  const int2* tiles;      // flash kernel: blockIdx.y -> (sequence, first query row of the 128-row tile within it)
  const int* row_seq;     // row kernel: blockIdx.y (a packed row) -> sequence
  int D, smax, H;
};
template <typename KVT, typename OT>
__device__ __forceinline__ AttnRowsArgs packed_seq_args(const AttnPackedArgs& p, int seq) {
  const PackSeq s = p.seqs[seq];
  const size_t slot_off = (size_t)s.slot * p.H * p.smax * HD;
  AttnRowsArgs a;
  a.q = p.q + (size_t)s.row0 * p.D;
  a.kcache = reinterpret_cast<const KVT*>(p.kcache) + slot_off;
  a.vcache = reinterpret_cast<const KVT*>(p.vcache) + slot_off;
  a.out = reinterpret_cast<OT*>(p.out) + (size_t)s.row0 * p.D;
  a.T = s.T; a.D = p.D; a.smax = p.smax; a.pos0 = s.pos0; a.valid_from = s.pos0;
  return a;
}

template <typename KVT, typename OT>
__global__ __launch_bounds__(256) void attn_rows_packed_kernel(AttnPackedArgs p) {  // grid (H, sum T)
  const int seq = p.row_seq[blockIdx.y];
  const AttnRowsArgs a = packed_seq_args<KVT, OT>(p, seq);
#define ROWS_ROW ((int)blockIdx.y - p.seqs[seq].row0)
#define ROWS_K0 0
#include "attn_rows_body.h"
#undef ROWS_ROW
#undef ROWS_K0
}

// A sequence of a latent pass (ixtts_gpt_latent_many) sits in the scratch slot at cache positions pos0 .., pos0 a multiple of 64 and
// not of attn_sweep's stride (NW * PPW * IT keys: 128 for fp32, 256 for 16-bit caches).  attn_sweep groups the keys of one softmax
// update by ABSOLUTE position, so at such a pos0 the kernel above would update in other groups than the solo pass at position 0 does
// and round differently.  This kernel hands the sweep the sequence's own keys as positions 0 .. (key offset pos0 = valid_from): the
// groups, masks and speculative first pass of the solo launch, whatever pos0 is.
template <typename KVT, typename OT>
__global__ __launch_bounds__(256) void attn_rows_packed_rebased_kernel(AttnPackedArgs p) {  // grid (H, sum T)
  const int seq = p.row_seq[blockIdx.y];
  const AttnRowsArgs a = packed_seq_args<KVT, OT>(p, seq);
#define ROWS_ROW ((int)blockIdx.y - p.seqs[seq].row0)
#define ROWS_K0 a.pos0
#include "attn_rows_body.h"
#undef ROWS_ROW
#undef ROWS_K0
}

// ---- the same attention as a causal flash kernel on the fp32 matrix cores (the latent pass: 1237 rows x 20 heads; the
// row-at-a-time kernel above re-streams every row's whole key prefix from L2: 94 GB per pass, 6.5 of its 10.4 ms).
// Structure of csrc/attn_full.hip (S^T = K Q^T leaves, in accumulator register r of lane l, the score of query l&31 against
// key (r&3)+8(r>>2)+4(l>>5), which is exactly the B operand of O^T += V^T P^T; one query column per lane, online softmax
// in per-lane scalars, scores in the log2 domain) plus: K/V come from the cache in its own type and are widened to fp32
// while staged; key k is visible to query row t iff valid_from <= k <= pos0 + t; a wave skips the tiles that lie
// entirely behind its last query's limit (it still keeps the workgroup's barriers).  One workgroup = 4 waves = 128 rows.
constexpr int FR_KT = 64, FR_KP = HD + 4;

template <typename KVT>
__device__ __forceinline__ void load_row16(const KVT* p, float (&v)[16]);
template <>
__device__ __forceinline__ void load_row16<float>(const float* p, float (&v)[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 t = reinterpret_cast<const float4*>(p)[i];
    v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
  }
}
template <>
__device__ __forceinline__ void load_row16<f16>(const f16* p, float (&v)[16]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint4 r = reinterpret_cast<const uint4*>(p)[i];
    v[8 * i] = lo_f16(r.x); v[8 * i + 1] = hi_f16(r.x); v[8 * i + 2] = lo_f16(r.y); v[8 * i + 3] = hi_f16(r.y);
    v[8 * i + 4] = lo_f16(r.z); v[8 * i + 5] = hi_f16(r.z); v[8 * i + 6] = lo_f16(r.w); v[8 * i + 7] = hi_f16(r.w);
  }
}
template <>
__device__ __forceinline__ void load_row16<bf16>(const bf16* p, float (&v)[16]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint4 r = reinterpret_cast<const uint4*>(p)[i];
    v[8 * i] = lo_bf16(r.x); v[8 * i + 1] = hi_bf16(r.x); v[8 * i + 2] = lo_bf16(r.y); v[8 * i + 3] = hi_bf16(r.y);
    v[8 * i + 4] = lo_bf16(r.z); v[8 * i + 5] = hi_bf16(r.z); v[8 * i + 6] = lo_bf16(r.w); v[8 * i + 7] = hi_bf16(r.w);
  }
}

// (the statements are attn_rows_flash_body.h, shared as text with attn_rows_flash_seq below)
template <typename KVT, typename OT>
__global__ __launch_bounds__(256) void attn_rows_flash_kernel(AttnRowsArgs a) {
#define FLASH_Q0 ((int)blockIdx.y * 128)
#include "attn_rows_flash_body.h"
#undef FLASH_Q0
}

// the same for one sequence of a packed pass: q0 is the first row of the workgroup's 128-row tile within the sequence
template <typename KVT, typename OT>
__device__ __forceinline__ void attn_rows_flash_seq(const AttnRowsArgs& a, const int q0) {
#define FLASH_Q0 q0
#include "attn_rows_flash_body.h"
#undef FLASH_Q0
}
template <typename KVT, typename OT>
__global__ __launch_bounds__(256) void attn_rows_flash_packed_kernel(AttnPackedArgs p) {  // grid (H, tiles of the pass)
  const int2 t = p.tiles[blockIdx.y];
  attn_rows_flash_seq<KVT, OT>(packed_seq_args<KVT, OT>(p, t.x), t.y);
}

static bool rows_attn_legacy() {  // IXTTS_ROWS_ATTN=legacy: the row-at-a-time kernels in place of the flash ones (A/B switch)
  static const bool legacy = getenv("IXTTS_ROWS_ATTN") && !strcmp(getenv("IXTTS_ROWS_ATTN"), "legacy");
  return legacy;
}

template <typename KVT, typename OT>
static void launch_attn_rows(ixtts_gpt* h, const AttnRowsArgs& a, hipStream_t st) {
  if (rows_attn_legacy()) hipLaunchKernelGGL((attn_rows_kernel<KVT, OT>), dim3(h->H, a.T), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((attn_rows_flash_kernel<KVT, OT>), dim3(h->H, ceil_div(a.T, 128)), dim3(256), 0, st, a);
}

// the packed pass's attention: one workgroup per (head, 128-row tile of ONE sequence) / per (head, packed row)
template <typename KVT, typename OT>
static void launch_attn_packed(ixtts_gpt* h, const PackedPass& pk, const void* kc_layer, const void* vc_layer, void* out, hipStream_t st) {
  const bool legacy = rows_attn_legacy();
  AttnPackedArgs p;
  p.q = h->rq; p.kcache = kc_layer; p.vcache = vc_layer; p.out = out; p.seqs = pk.seqs; p.tiles = reinterpret_cast<const int2*>(pk.tiles);
  p.row_seq = pk.row_seq; p.D = h->D; p.smax = h->smax; p.H = h->H;
  if (legacy && pk.keys_rebased) hipLaunchKernelGGL((attn_rows_packed_rebased_kernel<KVT, OT>), dim3(h->H, pk.T), dim3(256), 0, st, p);
  else if (legacy) hipLaunchKernelGGL((attn_rows_packed_kernel<KVT, OT>), dim3(h->H, pk.T), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((attn_rows_flash_packed_kernel<KVT, OT>), dim3(h->H, pk.n_tiles), dim3(256), 0, st, p);
}

// What the layer loop needs to know of a weight type: the GEMM's argument structs, the element type of the rows its producers
// (LayerNorm, attention, gelu) write into the workspaces, and the GEMM launch.
// bf16 / fp16 weights: rows of the weights' type (fp16 rows saturate at +-65504, store_kv), the LDS-DMA kernel on 128 x 128 tiles
template <typename WT, typename KVT>
struct RowsPath {
  typedef GemmArgs16 Args;
  typedef GemmArgs16Packed ArgsPacked;
  typedef KVT Act;
  template <int EPI, typename GA>
  static int gemm(const GA& g, hipStream_t st) {
    static const hipError_t attr = hipFuncSetAttribute((const void*)gemm_rows_bf16_kernel<EPI, KVT, GA>, hipFuncAttributeMaxDynamicSharedMemorySize, G16_SMEM);
    IX_HIP(attr);  // (once per kernel: the function is a template)
    hipLaunchKernelGGL((gemm_rows_bf16_kernel<EPI, KVT, GA>), dim3(ceil_div(g.N, 128), ceil_div(g.T, 128)), dim3(256), G16_SMEM, st, g);
    return IXTTS_OK;
  }
};
// fp32 weights: fp32 rows; 128-row tiles once there are enough rows to fill the GPU with them (latent pass), 64-row tiles for prompts
template <typename KVT>
struct RowsPath<float, KVT> {
  typedef GemmArgs Args;
  typedef GemmArgsPacked ArgsPacked;
  typedef float Act;
  template <int EPI, typename GA>
  static int gemm(const GA& g, hipStream_t st) {
    if (g.T >= 512) {
      hipLaunchKernelGGL((gemm_rows_kernel<float, EPI, KVT, 128, GA>), dim3(ceil_div(g.N, GBN), ceil_div(g.T, 128)), dim3(256), 0, st, g);
    } else {
      hipLaunchKernelGGL((gemm_rows_kernel<float, EPI, KVT, 64, GA>), dim3(ceil_div(g.N, GBN), ceil_div(g.T, 64)), dim3(256), 0, st, g);
    }
    return IXTTS_OK;
  }
};

// pk == nullptr: T rows of the sequence in `slot`.  pk: the packed rows of *pk (T = pk->T, slot 0 -- kc / vc are then the layer's
// bases, which is what the packed launches take -- pos0 and valid_from unused): the QKV GEMM and the attention take their packed
// forms, every other launch is the one-sequence launch at more rows.
template <typename WT, typename KVT, int D>
static int forward_rows_impl(ixtts_gpt* h, int slot, int T, int pos0, int valid_from, hipStream_t st, const PackedPass* pk) {
  using P = RowsPath<WT, KVT>;
  using Act = typename P::Act;
  const size_t lstride = (size_t)h->slots * D * h->smax * sizeof(KVT);
  const size_t sstride = (size_t)D * h->smax * sizeof(KVT);
  Act* xn = reinterpret_cast<Act*>(h->rxn);
  Act* att = reinterpret_cast<Act*>(h->ratt);
  Act* ff = reinterpret_cast<Act*>(h->rff);
  typename P::Args g;
  g.T = T; g.pos0 = pos0; g.smax = h->smax; g.D = D;
  auto operands = [&](const void* A, size_t w, size_t bias, void* out, int N, int K) {
    g.A = static_cast<decltype(g.A)>(A); g.wt = static_cast<decltype(g.wt)>(A_PTR(w)); g.bias = A_F32(bias);
    g.out = static_cast<decltype(g.out)>(out); g.N = N; g.K = K;
  };
  for (int l = 0; l < h->L; ++l) {
    const LayerOff& o = h->lo[l];
    uint8_t* kc = (uint8_t*)h->kc + l * lstride + slot * sstride;
    uint8_t* vc = (uint8_t*)h->vc + l * lstride + slot * sstride;
    hipLaunchKernelGGL((ln_rows_kernel<D, Act>), dim3(ceil_div(T, 4)), dim3(256), 0, st, h->rx, xn, T);
    operands(xn, o.wqkv, o.bqkv, h->rq, 3 * D, D);
    g.kcache = kc; g.vcache = vc;
    if (pk) {
      typename P::ArgsPacked gp;
      static_cast<typename P::Args&>(gp) = g;
      gp.row_at = pk->row_at;
      IX_TRY((P::template gemm<RE_QKV_PACKED>(gp, st)));
      launch_attn_packed<KVT, Act>(h, *pk, kc, vc, att, st);
    } else {
      IX_TRY((P::template gemm<RE_QKV>(g, st)));
      AttnRowsArgs a;
      a.q = h->rq; a.kcache = kc; a.vcache = vc; a.out = att; a.T = T; a.D = D; a.smax = h->smax; a.pos0 = pos0; a.valid_from = valid_from;
      launch_attn_rows<KVT, Act>(h, a, st);
    }
    operands(att, o.wo, o.bo, h->rx, D, D);
    IX_TRY((P::template gemm<RE_RESID>(g, st)));
    hipLaunchKernelGGL((ln_rows_kernel<D, Act>), dim3(ceil_div(T, 4)), dim3(256), 0, st, h->rx, xn, T);
    operands(xn, o.wfc, o.bfc, ff, 4 * D, D);
    IX_TRY((P::template gemm<RE_GELU>(g, st)));
    operands(ff, o.wpr, o.bpr, h->rx, D, 4 * D);
    IX_TRY((P::template gemm<RE_RESID>(g, st)));
  }
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

static int forward_rows_any(ixtts_gpt* h, int slot, int T, int pos0, int valid_from, hipStream_t st, const PackedPass* pk) {
  if (T <= 0) return IXTTS_OK;
  const bool wide = h->D == 1280;  // (create admits 1280 | 128)
  switch (h->cfg.weight_dtype) {
    case IXTTS_DTYPE_F32:
      return wide ? forward_rows_impl<float, float, 1280>(h, slot, T, pos0, valid_from, st, pk) : forward_rows_impl<float, float, 128>(h, slot, T, pos0, valid_from, st, pk);
    case IXTTS_DTYPE_F16:
      return wide ? forward_rows_impl<f16, f16, 1280>(h, slot, T, pos0, valid_from, st, pk) : forward_rows_impl<f16, f16, 128>(h, slot, T, pos0, valid_from, st, pk);
    default:
      return wide ? forward_rows_impl<bf16, bf16, 1280>(h, slot, T, pos0, valid_from, st, pk) : forward_rows_impl<bf16, bf16, 128>(h, slot, T, pos0, valid_from, st, pk);
  }
}

int forward_rows(ixtts_gpt* h, int slot, int T, int pos0, int valid_from, hipStream_t st) { return forward_rows_any(h, slot, T, pos0, valid_from, st, nullptr); }

int forward_rows_packed(ixtts_gpt* h, const PackedPass& p, hipStream_t st) { return forward_rows_any(h, 0, p.T, 0, 0, st, &p); }

// ---- packed pass, in and out.  One workgroup per packed row: row r of sequence s is the caller's embeds row pos0 + r, its last row
// the start-mel row mel_emb[start] + mel_pos[0] (the sum add_vec_kernel makes in ixtts_gpt_prefill: one fp32 add per element).
__global__ __launch_bounds__(256) void pack_rows_kernel(float* __restrict__ x, const PackSeq* __restrict__ seqs, const int* __restrict__ row_seq,
                                                         const float* __restrict__ start_emb, const float* __restrict__ mel_pos0, int D) {
  const int row = blockIdx.x;
  const PackSeq s = seqs[row_seq[row]];
  const int r = row - s.row0;
  float* dst = x + (size_t)row * D;
  if (r == s.T - 1) {
    for (int i = threadIdx.x; i < D; i += blockDim.x) dst[i] = start_emb[i] + mel_pos0[i];
  } else {
    const float* src = s.embeds + (size_t)(s.pos0 + r) * D;
    for (int i = threadIdx.x; i < D; i += blockDim.x) dst[i] = src[i];
  }
}
__global__ __launch_bounds__(256) void unpack_last_rows_kernel(float* __restrict__ hrow, const float* __restrict__ x, const PackSeq* __restrict__ seqs, int D) {
  const PackSeq s = seqs[blockIdx.x];
  const float* src = x + (size_t)(s.row0 + s.T - 1) * D;
  for (int i = threadIdx.x; i < D; i += blockDim.x) hrow[(size_t)s.slot * D + i] = src[i];
}

int pack_rows(ixtts_gpt* h, const PackedPass& p, hipStream_t st) {
  hipLaunchKernelGGL(pack_rows_kernel, dim3(p.T), dim3(256), 0, st, h->rx, p.seqs, p.row_seq,
                     (const float*)(A_F32(h->mel_emb) + (size_t)h->cfg.start_mel_token * h->D), (const float*)A_F32(h->mel_pos), h->D);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}
int unpack_last_rows(ixtts_gpt* h, const PackedPass& p, hipStream_t st) {
  hipLaunchKernelGGL(unpack_last_rows_kernel, dim3(p.n_seq), dim3(256), 0, st, h->h, (const float*)h->rx, p.seqs, h->D);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

int final_norm_rows(ixtts_gpt* h, const float* x, float* y, int T, hipStream_t st) {
  if (T <= 0) return IXTTS_OK;
  if (h->D == 1280)
    hipLaunchKernelGGL(final_norm_rows_kernel<1280>, dim3(ceil_div(T, 4)), dim3(256), 0, st, x, y, T, (const float*)A_F32(h->lnf_w),
                       (const float*)A_F32(h->lnf_b), (const float*)A_F32(h->fn_w), (const float*)A_F32(h->fn_b));
  else
    hipLaunchKernelGGL(final_norm_rows_kernel<128>, dim3(ceil_div(T, 4)), dim3(256), 0, st, x, y, T, (const float*)A_F32(h->lnf_w),
                       (const float*)A_F32(h->lnf_b), (const float*)A_F32(h->fn_w), (const float*)A_F32(h->fn_b));
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

// rows of [start, codes...] embedded with mel positions 0..: x[r] = mel_emb[tok] + mel_pos[r]
__global__ void embed_mel_rows_kernel(float* x, const float* mel_emb, const float* mel_pos, const int32_t* codes, int start_tok,
                                      int rows, int D) {
  const int r = blockIdx.x;
  if (r >= rows) return;
  const int tok = (r == 0) ? start_tok : codes[r - 1];
  for (int i = threadIdx.x; i < D; i += blockDim.x) x[(size_t)r * D + i] = mel_emb[(size_t)tok * D + i] + mel_pos[(size_t)r * D + i];
}

int embed_mel_rows(ixtts_gpt* h, float* x, const int32_t* codes, int rows, hipStream_t st) {
  if (rows <= 0) return IXTTS_OK;
  hipLaunchKernelGGL(embed_mel_rows_kernel, dim3(rows), dim3(256), 0, st, x, (const float*)A_F32(h->mel_emb), (const float*)A_F32(h->mel_pos), codes,
                     h->cfg.start_mel_token, rows, h->D);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

// ---- latent pass of several sequences (ixtts_gpt_latent_many), in and out.  In: one workgroup per packed row, the launch shape of
// embed_mel_rows_kernel; row r of a sequence is its prefix row r, or from r = n_prefix on the mel row m = r - n_prefix:
// mel_emb[m == 0 ? start : codes[m - 1]] + mel_pos[m], the one fp32 add embed_mel_rows_kernel makes.
__global__ __launch_bounds__(256) void latent_pack_rows_kernel(float* __restrict__ x, const PackSeq* __restrict__ seqs, const LatentSeq* __restrict__ lseqs,
                                                                const int* __restrict__ row_seq, const float* __restrict__ mel_emb,
                                                                const float* __restrict__ mel_pos, int start_tok, int D) {
  const int row = blockIdx.x;
  const int q = row_seq[row];
  const LatentSeq e = lseqs[q];
  const int r = row - seqs[q].row0;
  float* dst = x + (size_t)row * D;
  if (r < e.n_prefix) {
    const float* src = e.prefix + (size_t)r * D;
    for (int i = threadIdx.x; i < D; i += blockDim.x) dst[i] = src[i];
  } else {
    const int m = r - e.n_prefix;
    const int tok = (m == 0) ? start_tok : e.codes[m - 1];
    for (int i = threadIdx.x; i < D; i += blockDim.x) dst[i] = mel_emb[(size_t)tok * D + i] + mel_pos[(size_t)m * D + i];
  }
}
// Out: one wave per mel row of the pass, the launch shape of final_norm_rows_kernel and its row arithmetic (final_norm_row)
template <int K>
__global__ __launch_bounds__(256) void latent_norm_scatter_kernel(const float* __restrict__ x, const PackSeq* __restrict__ seqs,
                                                                   const LatentSeq* __restrict__ lseqs, const int* __restrict__ row_seq,
                                                                   const int* __restrict__ mel_row, int n_mel, const float* __restrict__ w1,
                                                                   const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= n_mel) return;
  const int row = mel_row[m];
  const int q = row_seq[row];
  const LatentSeq e = lseqs[q];
  final_norm_row<K>(x, e.latent, (size_t)row, (size_t)(row - seqs[q].row0 - e.n_prefix), lane, w1, b1, w2, b2);
}

int pack_latent_rows(ixtts_gpt* h, const PackedPass& p, const LatentPass& lp, hipStream_t st) {
  if (p.T <= 0) return IXTTS_OK;
  hipLaunchKernelGGL(latent_pack_rows_kernel, dim3(p.T), dim3(256), 0, st, h->rx, p.seqs, lp.lseqs, p.row_seq, (const float*)A_F32(h->mel_emb),
                     (const float*)A_F32(h->mel_pos), h->cfg.start_mel_token, h->D);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}
int scatter_latent_rows(ixtts_gpt* h, const PackedPass& p, const LatentPass& lp, hipStream_t st) {
  if (lp.n_mel <= 0) return IXTTS_OK;
  if (h->D == 1280)
    hipLaunchKernelGGL(latent_norm_scatter_kernel<1280>, dim3(ceil_div(lp.n_mel, 4)), dim3(256), 0, st, (const float*)h->rx, p.seqs, lp.lseqs, p.row_seq, lp.mel_row,
                       lp.n_mel, (const float*)A_F32(h->lnf_w), (const float*)A_F32(h->lnf_b), (const float*)A_F32(h->fn_w), (const float*)A_F32(h->fn_b));
  else
    hipLaunchKernelGGL(latent_norm_scatter_kernel<128>, dim3(ceil_div(lp.n_mel, 4)), dim3(256), 0, st, (const float*)h->rx, p.seqs, lp.lseqs, p.row_seq, lp.mel_row,
                       lp.n_mel, (const float*)A_F32(h->lnf_w), (const float*)A_F32(h->lnf_b), (const float*)A_F32(h->fn_w), (const float*)A_F32(h->fn_b));
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

}  // namespace ixtts
