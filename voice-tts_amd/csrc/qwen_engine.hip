// qwen_engine.hip -- the Qwen3 causal LM of the text-emotion model (QwenEmotion, indextts/infer_v2.py:795-906), decoded
// on gfx950: 1..IXTTS_QWEN_MAX_SLOTS sequences ("slots") per engine.  Slot 0 is the sequence of the one-sequence calls.
//
// One decode step = 5 launches per layer + 3:
//   L x { RMSNorm (in the staging of x) + q|k|v GEMV   [layer 0: the embedding row gather is that staging]
//       | q_norm / k_norm + RoPE + K/V append + split-S GQA attention (each K/V row read once for its query heads)
//       | merge of the splits (in the staging) + o_proj GEMV + residual
//       | RMSNorm (staging) + gate|up GEMV + SiLU(gate) * up
//       | down GEMV + residual }
//   -> norm (staging) + lm_head GEMV -> top-k candidates per workgroup -> one merge + temperature / top-p / draw.
// Prefill runs the layers over PCH prompt positions per step: the same GEMVs with PCH columns (one pass over the weights),
// q/k norm + RoPE + K/V append of the PCH positions (qprep), and a causal attention of the PCH queries over the cache.
// B = 1 is launch-chain bound, so the kernels are few and every GEMV streams its weights with the
// 16-byte non-temporal loads of the GPT engine (load_w16), all of a wave's chunks in flight before the staging of x where
// they fit in registers (the layer GEMVs in f16), else one chunk ahead of the arithmetic.  The token, the position
// and the sampling parameters live on the device: a captured chain replays for any step.
//
// Slots: a decode step of n slots is the same chain with column c of the GEMVs being slot c (its own token, position,
// K/V cache, logits row and token selection), so slot c's arithmetic is the one-sequence step's, bit for bit.  On f16
// engines the prompts of a batch are prefilled as rows: every prompt position of every slot is one row of fp32 activations,
// and the layer matrices are GEMMs on v_mfma_f32_32x32x16_f16 (qrows_*; one pass over the weights for the whole batch).
//
// Arithmetic: transformers/models/qwen3/modeling_qwen3.py (Qwen3RMSNorm, Qwen3Attention, Qwen3MLP, rotate_half RoPE with
// inv_freq = 1 / theta^(2i/d), scaling = head_dim^-0.5); token selection: TemperatureLogitsWarper -> TopKLogitsWarper ->
// TopPLogitsWarper -> multinomial (transformers generation/logits_process.py).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "gpt_kernels.h"

namespace ixtts {
namespace qw {

constexpr int HDIM = 128;      // head_dim (the only one built)
constexpr int NSP = 8;         // attention splits per KV head (contiguous key ranges)
constexpr int PSTR = 2 + HDIM; // partial of one (query head, split): max, sum, acc[HDIM]
constexpr int WAVES = 4;       // GEMV workgroup = 4 independent waves
constexpr int PRE = 6;         // weight chunks a wave of the 2-row GEMVs has in flight before its first FMA
constexpr int SAMP_WG = 128;   // first-pass sampler workgroups
constexpr int SAMP_CHUNK = 2048;
constexpr int KC_MAX = IXTTS_QWEN_TOPK_MAX;
constexpr int STEPS_PER_GRAPH = 8;
constexpr int PCH = 4;  // prompt positions per prefill step (one weight pass for all of them)

typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

template <typename WT>
struct WV;
template <>
struct WV<float> {
  static constexpr int VEC = 4;
  __device__ static __forceinline__ void unpack(const uint4& r, float (&w)[4]) {
    w[0] = __uint_as_float(r.x), w[1] = __uint_as_float(r.y), w[2] = __uint_as_float(r.z), w[3] = __uint_as_float(r.w);
  }
};
template <>
struct WV<_Float16> {
  static constexpr int VEC = 8;
  __device__ static __forceinline__ void unpack(const uint4& r, float (&w)[8]) {
    const h8_t v = __builtin_bit_cast(h8_t, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = (float)v[i];
  }
};

struct SampDev {
  float temperature, top_p;
  int do_sample, top_k, kc;  // kc: candidates per first-pass workgroup (1 greedy, else the power of two >= top_k)
  unsigned long long seed;
};

enum { PRO_PLAIN = 0, PRO_NORM = 1, PRO_EMBED = 2, PRO_MERGE = 3 };
enum { EPI_STORE = 0, EPI_ADD = 1, EPI_SWIGLU = 2 };

struct GemvP {
  const void* w;  // [rows][K] (HF Linear layout); EPI_SWIGLU: gate rows [0, N) then up rows [N, 2N)
  int N, K;       // outputs, reduction length
  const float* x; // PRO_PLAIN / PRO_NORM input [K]
  const float* g; // RMSNorm weight [K]
  float eps;
  float* out;
  const void* emb;  // PRO_EMBED: embedding table [V][K] (weight dtype), row tokens[*cur_len]; block 0 writes it to h_out
  const int32_t* tokens;
  const int* cur_len;
  float* h_out;
  const float* part;  // PRO_MERGE: [heads][NSP][PSTR]
  int* advance;       // non-null: block 0 increments it at the end (a prefill step moves the position)
  int slots, tstride; // slots != 0: column c is slot c, PRO_EMBED gathers tokens[c * tstride + cur_len[c]]
  int nact;           // columns [nact, NC) are idle (a step of 3 slots on the 4-column kernel): computed, never stored
};

// ---- GEMV: stage x (optionally normalised / gathered / merged) in LDS, then each wave streams ROWS weight rows.
// ROWS = 2 (the layer GEMVs): every chunk of the wave's rows is loaded before the prologue when K <= 64 * VEC * PRE (f16: K <= 3072),
// so a launch costs one memory latency, not one per chunk; ROWS = 4 (lm_head, 151 936 rows: fewer copies of the prologue) and
// longer rows keep one chunk ahead of the FMAs.  NC columns (prefill chunks: NC consecutive positions) share each weight load:
// x, out and the attention partials are [NC][.] with strides K, N and heads * NSP * PSTR.
template <typename WT, int PRO, int EPI, int ROWS, int NC>
__global__ __launch_bounds__(64 * WAVES) void qgemv_kernel(GemvP p) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  __shared__ float red[WAVES][NC];
  constexpr int VEC = WV<WT>::VEC;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, N = p.N;
  const int nch = K / (64 * VEC);  // K % 512 == 0 (checked at create)
  const int unit = blockIdx.x * WAVES + wave;
  const char* wb = reinterpret_cast<const char*>(p.w);
  size_t roff[ROWS];
  bool rok[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    int row, o;
    if constexpr (EPI == EPI_SWIGLU) {
      o = unit * (ROWS / 2) + (r >> 1);
      row = (r & 1) * N + min(o, N - 1);
    } else {
      o = unit * ROWS + r;
      row = min(o, N - 1);
    }
    rok[r] = o < N;
    roff[r] = (size_t)row * K * sizeof(WT) + (size_t)lane * VEC * sizeof(WT);
  }
  constexpr int NPRE = ROWS == 2 ? PRE : 1;
  const int npre = min(nch, NPRE);
  constexpr size_t CB = 64 * VEC * sizeof(WT);  // bytes of one chunk of a row
  // these chunks of weights fly while x is staged
  uint4 wr[NPRE][ROWS];
#pragma unroll
  for (int c = 0; c < NPRE; ++c)
    if (c < npre)
#pragma unroll
      for (int r = 0; r < ROWS; ++r) wr[c][r] = load_w16(wb + roff[r] + c * CB);
  // ---- prologue
  if constexpr (PRO == PRO_PLAIN) {
    for (int k = tid; k < NC * K; k += 64 * WAVES) xs[k] = p.x[k];
    __syncthreads();
  } else if constexpr (PRO == PRO_MERGE) {
    const size_t cstride = (size_t)(K / HDIM) * NSP * PSTR;
    for (int ck = tid; ck < NC * K; ck += 64 * WAVES) {
      const int c = ck / K, k = ck % K;
      const float* pp = p.part + c * cstride + (size_t)(k / HDIM) * NSP * PSTR;
      float M = -INFINITY;
#pragma unroll
      for (int s = 0; s < NSP; ++s) M = fmaxf(M, pp[s * PSTR]);
      float num = 0.f, den = 0.f;
#pragma unroll
      for (int s = 0; s < NSP; ++s) {
        const float m = pp[s * PSTR];
        const float e = m == -INFINITY ? 0.f : expf(m - M);
        den = fmaf(e, pp[s * PSTR + 1], den);
        num = fmaf(e, pp[s * PSTR + 2 + (k % HDIM)], num);
      }
      xs[ck] = num / den;
    }
    __syncthreads();
  } else {
    float ss[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      ss[c] = 0.f;
      if constexpr (PRO == PRO_EMBED) {
        const int tok = p.slots ? p.tokens[(size_t)c * p.tstride + p.cur_len[c]] : p.tokens[*p.cur_len + c];
        const WT* e = reinterpret_cast<const WT*>(p.emb) + (size_t)tok * K;
        for (int k = tid; k < K; k += 64 * WAVES) {
          const float v = (float)e[k];
          xs[c * K + k] = v;
          ss[c] = fmaf(v, v, ss[c]);
          if (blockIdx.x == 0 && c < p.nact) p.h_out[c * K + k] = v;
        }
      } else {
        for (int k = tid; k < K; k += 64 * WAVES) {
          const float v = p.x[c * K + k];
          xs[c * K + k] = v;
          ss[c] = fmaf(v, v, ss[c]);
        }
      }
      ss[c] = wave_sum(ss[c]);
      if (lane == 0) red[wave][c] = ss[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) tot += red[w][c];
      const float rs = rsqrtf(tot / (float)K + p.eps);
      for (int k = tid; k < K; k += 64 * WAVES) xs[c * K + k] = p.g[k] * (xs[c * K + k] * rs);  // Qwen3RMSNorm: weight * (x * rsqrt(var + eps))
    }
    __syncthreads();
  }
  // ---- dot products: the preloaded chunks, then the rest one chunk ahead
  float acc[ROWS][NC];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[r][c] = 0.f;
  auto dot = [&](const uint4 (&w)[ROWS], int ch) {
    const int k0 = ch * 64 * VEC + lane * VEC;
    float wv[ROWS][VEC];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) WV<WT>::unpack(w[r], wv[r]);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float xv[VEC];
#pragma unroll
      for (int i = 0; i < VEC; i += 4) {
        const float4 t = *reinterpret_cast<const float4*>(&xs[c * K + k0 + i]);
        xv[i] = t.x, xv[i + 1] = t.y, xv[i + 2] = t.z, xv[i + 3] = t.w;
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[r][c] = fmaf(wv[r][i], xv[i], acc[r][c]);
    }
  };
#pragma unroll
  for (int c = 0; c < NPRE; ++c)
    if (c < npre) dot(wr[c], c);
  if (nch > NPRE) {
    uint4 nxt[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) nxt[r] = load_w16(wb + roff[r] + NPRE * CB);
    for (int c = NPRE; c < nch; ++c) {
      uint4 cur[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) cur[r] = nxt[r];
      const size_t nx = (size_t)min(c + 1, nch - 1) * CB;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) nxt[r] = load_w16(wb + roff[r] + nx);
      dot(cur, c);
    }
  }
  float tot[ROWS][NC];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int c = 0; c < NC; ++c) tot[r][c] = wave_sum(acc[r][c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c >= p.nact) continue;
      float* out = p.out + (size_t)c * N;
      if constexpr (EPI == EPI_SWIGLU) {
#pragma unroll
        for (int j = 0; j < ROWS / 2; ++j) {
          const int o = unit * (ROWS / 2) + j;
          const float g = tot[2 * j][c], u = tot[2 * j + 1][c];
          if (rok[2 * j]) out[o] = g / (1.f + expf(-g)) * u;
        }
      } else {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          const int o = unit * ROWS + r;
          if (rok[r]) {
            if constexpr (EPI == EPI_ADD) out[o] += tot[r][c];
            else out[o] = tot[r][c];
          }
        }
      }
    }
  }
  if (p.advance && blockIdx.x == 0 && tid == 0) *p.advance += NC;
}

// ---- attention.  grid (kv_heads, NSP, slots): split sp owns keys [sp*ch, min((sp+1)*ch, pos+1)), ch = ceil((pos+1)/NSP).
// Prologue: q_norm + RoPE of the NREP query heads of this KV head (every workgroup), k_norm + RoPE of the new key and the
// new value (the workgroup whose range holds `pos`: it appends them to the cache and reads them from LDS).
// Slot z takes qkv / part of column z, cur_len[z] and its own cache; a finished slot's new key and value stay in LDS.
constexpr int MAXS = IXTTS_QWEN_MAX_SLOTS;
static_assert(MAXS == PCH, "a decode step of all slots is the PCH-column GEMV");
struct AttnP {
  const float* qkv;  // raw projections [heads*HDIM | kv_heads*HDIM | kv_heads*HDIM] per column
  const float *qn, *kn;  // q_norm / k_norm weights [HDIM]
  const float *cosb, *sinb;  // [max_seq][HDIM/2]
  float *kc[MAXS], *vc[MAXS];  // this layer's cache of each slot [kv_heads][smax][HDIM] (the chunk path: [0])
  const int* cur_len;  // [slots]
  const int* finished;  // slots path: [slots]; null: always append
  float* part;       // [heads][NSP][PSTR] per column
  int heads, kv_heads, smax;
  float eps, scale;
  float* qb;        // prefill chunks: q_norm + RoPE of [PCH][heads][HDIM]
};

__device__ __forceinline__ void norm_rope_head(const float* x, const float* w, const float* cs, const float* sn, float eps, bool rope,
                                               int lane, float* out) {
  const float a = x[lane], b = x[lane + 64];
  const float ss = wave_sum(fmaf(a, a, b * b));
  const float rs = rsqrtf(ss / (float)HDIM + eps);
  const float ya = w[lane] * (a * rs), yb = w[lane + 64] * (b * rs);
  if (rope) {
    // q * cos + rotate_half(q) * sin, rotate_half = cat(-x2, x1); cos/sin repeat over the two halves
    const float c = cs[lane], s = sn[lane];
    out[lane] = ya * c - yb * s;
    out[lane + 64] = yb * c + ya * s;
  } else {
    out[lane] = ya;
    out[lane + 64] = yb;
  }
}

// p[slot] without a run-time index into the kernel argument (which would move the whole argument to scratch)
template <typename PT>
__device__ __forceinline__ PT pick_slot(PT const (&p)[MAXS], int slot) {
  return slot == 0 ? p[0] : slot == 1 ? p[1] : slot == 2 ? p[2] : p[3];
}

template <int NREP>
__global__ __launch_bounds__(256) void qattn_kernel(AttnP p) {
  __shared__ __attribute__((aligned(16))) float qs[NREP][HDIM];
  __shared__ __attribute__((aligned(16))) float knew[HDIM], vnew[HDIM];
  __shared__ float gm[16][NREP], gl[16][NREP];
  __shared__ __attribute__((aligned(16))) float gacc[16][NREP][HDIM];
  const int kvh = blockIdx.x, sp = blockIdx.y, slot = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pos = p.cur_len[slot];
  const int n = pos + 1, ch = (n + NSP - 1) / NSP;
  const int lo = sp * ch, hi = min(n, lo + ch);
  const bool owner = lo <= pos && pos < hi;
  const bool append = p.finished == nullptr || p.finished[slot] == 0;
  const float* const qkv = p.qkv + (size_t)slot * (p.heads + 2 * p.kv_heads) * HDIM;
  float* const part = p.part + (size_t)slot * p.heads * NSP * PSTR;
  float* const kcache = pick_slot(p.kc, slot);
  float* const vcache = pick_slot(p.vc, slot);
  const float* cs = p.cosb + (size_t)pos * (HDIM / 2);
  const float* sn = p.sinb + (size_t)pos * (HDIM / 2);
  const int qdim = p.heads * HDIM, kvdim = p.kv_heads * HDIM;
  for (int j = wave; j < NREP + 2; j += 4) {
    if (j < NREP) {
      norm_rope_head(qkv + (size_t)(kvh * NREP + j) * HDIM, p.qn, cs, sn, p.eps, true, lane, qs[j]);
    } else if (owner && j == NREP) {
      norm_rope_head(qkv + qdim + (size_t)kvh * HDIM, p.kn, cs, sn, p.eps, true, lane, knew);
      if (append) {
        float* kd = kcache + ((size_t)kvh * p.smax + pos) * HDIM;
        kd[lane] = knew[lane];
        kd[lane + 64] = knew[lane + 64];
      }
    } else if (owner) {
      const float* v = qkv + qdim + kvdim + (size_t)kvh * HDIM;
      vnew[lane] = v[lane];
      vnew[lane + 64] = v[lane + 64];
      if (append) {
        float* vd = vcache + ((size_t)kvh * p.smax + pos) * HDIM;
        vd[lane] = v[lane];
        vd[lane + 64] = v[lane + 64];
      }
    }
  }
  __syncthreads();
  // 16 lane groups of 16 lanes; lane dl of a group holds dims [8 dl, 8 dl + 8) of a key
  const int g = tid >> 4, dl = tid & 15;
  float q[NREP][8];
#pragma unroll
  for (int j = 0; j < NREP; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) q[j][i] = qs[j][dl * 8 + i];
  float m[NREP], l[NREP], acc[NREP][8];
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    m[j] = -INFINITY, l[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = 0.f;
  }
  const float* kb = kcache + (size_t)kvh * p.smax * HDIM + dl * 8;
  const float* vb = vcache + (size_t)kvh * p.smax * HDIM + dl * 8;
  for (int key = lo + g; key < hi; key += 16) {
    float kv[8], vv[8];
    if (key == pos) {
#pragma unroll
      for (int i = 0; i < 8; ++i) kv[i] = knew[dl * 8 + i], vv[i] = vnew[dl * 8 + i];
    } else {
      const float4 k0 = *reinterpret_cast<const float4*>(kb + (size_t)key * HDIM);
      const float4 k1 = *reinterpret_cast<const float4*>(kb + (size_t)key * HDIM + 4);
      const float4 v0 = *reinterpret_cast<const float4*>(vb + (size_t)key * HDIM);
      const float4 v1 = *reinterpret_cast<const float4*>(vb + (size_t)key * HDIM + 4);
      kv[0] = k0.x, kv[1] = k0.y, kv[2] = k0.z, kv[3] = k0.w, kv[4] = k1.x, kv[5] = k1.y, kv[6] = k1.z, kv[7] = k1.w;
      vv[0] = v0.x, vv[1] = v0.y, vv[2] = v0.z, vv[3] = v0.w, vv[4] = v1.x, vv[5] = v1.y, vv[6] = v1.z, vv[7] = v1.w;
    }
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) d = fmaf(q[j][i], kv[i], d);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) d += __shfl_xor(d, o, 64);
      const float s = d * p.scale;
      const float mn = fmaxf(m[j], s);
      const float a = expf(m[j] - mn), e = expf(s - mn);  // m = -inf on the first key: a = 0
      l[j] = fmaf(l[j], a, e);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j][i] = fmaf(acc[j][i], a, e * vv[i]);
      m[j] = mn;
    }
  }
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    if (dl == 0) gm[g][j] = m[j], gl[g][j] = l[j];
#pragma unroll
    for (int i = 0; i < 8; ++i) gacc[g][j][dl * 8 + i] = acc[j][i];
  }
  __syncthreads();
  for (int t = tid; t < NREP * HDIM; t += 256) {
    const int j = t / HDIM, d = t % HDIM;
    float M = -INFINITY;
#pragma unroll
    for (int gg = 0; gg < 16; ++gg) M = fmaxf(M, gm[gg][j]);
    float o = 0.f, L = 0.f;
    if (M > -INFINITY) {
#pragma unroll
      for (int gg = 0; gg < 16; ++gg) {
        const float e = gm[gg][j] == -INFINITY ? 0.f : expf(gm[gg][j] - M);
        o = fmaf(e, gacc[gg][j][d], o);
        L = fmaf(e, gl[gg][j], L);
      }
    }
    float* pp = part + ((size_t)(kvh * NREP + j) * NSP + sp) * PSTR;
    pp[2 + d] = o;
    if (d == 0) pp[0] = M, pp[1] = L;  // an empty split: M = -inf, L = 0, the merge gives it weight 0
  }
}

// ---- prefill chunks of PCH positions cur_len .. cur_len + PCH - 1.  qprep: q_norm / k_norm + RoPE of every position, K/V appended
// (grid (PCH, heads + kv_heads), one wave each); then causal attention of the PCH queries over the cache.
__global__ __launch_bounds__(64) void qprep_kernel(AttnP p) {
  const int c = blockIdx.x, hh = blockIdx.y, lane = threadIdx.x;
  const int pos = *p.cur_len + c;
  const float* cs = p.cosb + (size_t)pos * (HDIM / 2);
  const float* sn = p.sinb + (size_t)pos * (HDIM / 2);
  const int qdim = p.heads * HDIM, kvdim = p.kv_heads * HDIM;
  const float* x = p.qkv + (size_t)c * (qdim + 2 * kvdim);
  if (hh < p.heads) {
    norm_rope_head(x + (size_t)hh * HDIM, p.qn, cs, sn, p.eps, true, lane, p.qb + ((size_t)c * p.heads + hh) * HDIM);
  } else {
    const int kvh = hh - p.heads;
    norm_rope_head(x + qdim + (size_t)kvh * HDIM, p.kn, cs, sn, p.eps, true, lane, p.kc[0] + ((size_t)kvh * p.smax + pos) * HDIM);
    const float* v = x + qdim + kvdim + (size_t)kvh * HDIM;
    float* vd = p.vc[0] + ((size_t)kvh * p.smax + pos) * HDIM;
    vd[lane] = v[lane];
    vd[lane + 64] = v[lane + 64];
  }
}

template <int NREP>
__global__ __launch_bounds__(256) void qattn_chunk_kernel(AttnP p) {
  constexpr int NQ = PCH * NREP;
  __shared__ float gm[16][2], gl[16][2];
  __shared__ __attribute__((aligned(16))) float gacc[16][2][HDIM];
  const int kvh = blockIdx.x, sp = blockIdx.y;
  const int tid = threadIdx.x;
  const int p0 = *p.cur_len;
  const int n = p0 + PCH, ch = (n + NSP - 1) / NSP;
  const int lo = sp * ch, hi = min(n, lo + ch);
  const int g = tid >> 4, dl = tid & 15;
  float q[NQ][8], m[NQ], l[NQ], acc[NQ][8];
#pragma unroll
  for (int c = 0; c < PCH; ++c)
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      const float* qp = p.qb + ((size_t)c * p.heads + kvh * NREP + j) * HDIM + dl * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i) q[c * NREP + j][i] = qp[i], acc[c * NREP + j][i] = 0.f;
      m[c * NREP + j] = -INFINITY, l[c * NREP + j] = 0.f;
    }
  const float* kb = p.kc[0] + (size_t)kvh * p.smax * HDIM + dl * 8;
  const float* vb = p.vc[0] + (size_t)kvh * p.smax * HDIM + dl * 8;
  for (int key = lo + g; key < hi; key += 16) {
    const float4 k0 = *reinterpret_cast<const float4*>(kb + (size_t)key * HDIM);
    const float4 k1 = *reinterpret_cast<const float4*>(kb + (size_t)key * HDIM + 4);
    const float4 v0 = *reinterpret_cast<const float4*>(vb + (size_t)key * HDIM);
    const float4 v1 = *reinterpret_cast<const float4*>(vb + (size_t)key * HDIM + 4);
    const float kv[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
    const float vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int c = 0; c < PCH; ++c) {
      if (key > p0 + c) continue;  // causal: the same for the 16 lanes of a key
#pragma unroll
      for (int j = 0; j < NREP; ++j) {
        const int qi = c * NREP + j;
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d = fmaf(q[qi][i], kv[i], d);
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) d += __shfl_xor(d, o, 64);
        const float sc = d * p.scale;
        const float mn = fmaxf(m[qi], sc);
        const float a = expf(m[qi] - mn), e = expf(sc - mn);
        l[qi] = fmaf(l[qi], a, e);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[qi][i] = fmaf(acc[qi][i], a, e * vv[i]);
        m[qi] = mn;
      }
    }
  }
  // the 16 lane groups merged through LDS, two queries per round
#pragma unroll
  for (int q0 = 0; q0 < NQ; q0 += 2) {
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      if (dl == 0) gm[g][jj] = m[q0 + jj], gl[g][jj] = l[q0 + jj];
#pragma unroll
      for (int i = 0; i < 8; ++i) gacc[g][jj][dl * 8 + i] = acc[q0 + jj][i];
    }
    __syncthreads();
    const int jj = tid / HDIM, d = tid % HDIM;  // 256 threads = 2 queries x HDIM
    float M = -INFINITY;
#pragma unroll
    for (int gg = 0; gg < 16; ++gg) M = fmaxf(M, gm[gg][jj]);
    float o = 0.f, L = 0.f;
    if (M > -INFINITY) {
#pragma unroll
      for (int gg = 0; gg < 16; ++gg) {
        const float e = gm[gg][jj] == -INFINITY ? 0.f : expf(gm[gg][jj] - M);
        o = fmaf(e, gacc[gg][jj][d], o);
        L = fmaf(e, gl[gg][jj], L);
      }
    }
    const int qi = q0 + jj, c = qi / NREP, j = qi % NREP;
    float* pp = p.part + (((size_t)c * p.heads + kvh * NREP + j) * NSP + sp) * PSTR;
    pp[2 + d] = o;
    if (d == 0) pp[0] = M, pp[1] = L;
  }
}

// ---- rows prefill (f16 engines): every prompt position of every slot of a batch is one row.  row_slot / row_pos name the
// row's sequence and position; rows are packed in (slot, position) order, so a pass of at most rows_max rows finds the
// keys of earlier passes in the cache.
struct RowsP {
  const int *row_slot, *row_pos;  // [M]
  int M;
};

// x[row] = embedding row of the row's token (grid M)
__global__ __launch_bounds__(256) void qrows_embed_kernel(RowsP r, const _Float16* emb, const int32_t* tokens, int tstride, int K, float* x) {
  const int row = blockIdx.x;
  const int tok = tokens[(size_t)r.row_slot[row] * tstride + r.row_pos[row]];
  const _Float16* e = emb + (size_t)tok * K;
  for (int k = threadIdx.x; k < K; k += 256) x[(size_t)row * K + k] = (float)e[k];
}

// Qwen3RMSNorm of each row (grid M): y = weight * (x * rsqrt(mean(x^2) + eps))
__global__ __launch_bounds__(256) void qrows_norm_kernel(const float* x, const float* g, float eps, int K, float* y) {
  __shared__ float red[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* xr = x + (size_t)row * K;
  float ss = 0.f;
  for (int k = tid; k < K; k += 256) ss = fmaf(xr[k], xr[k], ss);
  ss = wave_sum(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  const float rs = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K + eps);
  for (int k = tid; k < K; k += 256) y[(size_t)row * K + k] = g[k] * (xr[k] * rs);
}

// GEMM of the rows: C[M][N] (+)= A[M][K] . W[N][K]^T, A fp32 rows, W the f16 arena in the layout the GEMVs stream.
// Tile 64 x 128 x 64, 4 waves as 2 x 2, wave tile 32 x 64 on v_mfma_f32_32x32x16_f16.  The staging pass writes an A tile as two
// f16 planes, hi = f16(a) and lo = f16(a - hi): f16 x f16 products are exact in the fp32 accumulator, so hi.W + lo.W
// carries ~22 bits of the activation and the result differs from the GEMV path by the order of the sums (the
// split-product idea of DESIGN.md 4.4 with the weight side already exact).  |a| saturates at the f16 maximum.  LDS rows
// are padded to 144 bytes: the 16-byte fragment reads of 8 consecutive rows fall in 8 different bank groups.  The
// global loads of k-tile i+1 are issued before the MFMAs of k-tile i and written to LDS after them.
// RE_SWIGLU: N = intermediate size; W holds gate rows [0, N) then up rows [N, 2N); a workgroup computes 64 outputs, wave
// column block j = 0 the gate and j = 1 the up of the same outputs, out = SiLU(gate) * up.
enum { RE_STORE = 0, RE_ADD = 1, RE_SWIGLU = 2 };
constexpr int RBM = 64, RBN = 128, RBK = 64, RPITCH = RBK + 8;  // pitch in halfs
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct RGemmP {
  const float* A;     // [M][K]
  const _Float16* W;  // [N][K] (RE_SWIGLU: [2N][K])
  float* out;         // [M][N]
  int M, N, K;
};

template <int EPI>
__global__ __launch_bounds__(256) void qrows_gemm_kernel(RGemmP g) {
  __shared__ __attribute__((aligned(16))) _Float16 Ah[RBM * RPITCH];
  __shared__ __attribute__((aligned(16))) _Float16 Al[RBM * RPITCH];
  __shared__ __attribute__((aligned(16))) _Float16 Ws[RBN * RPITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.y * RBM;
  const int n0 = blockIdx.x * (EPI == RE_SWIGLU ? RBN / 2 : RBN);

  f32x16_t acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  constexpr int NA = RBM * RBK / 4 / 256;  // float4 of A per thread per k-tile
  constexpr int NW = RBN * RBK / 8 / 256;  // 16-byte pieces of W per thread
  constexpr int AC = RBK / 4, WC = RBK / 8;
  const float* asrc[NA];
  const _Float16* wsrc[NW];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int idx = tid + i * 256;
    asrc[i] = g.A + (size_t)min(m0 + idx / AC, g.M - 1) * g.K + (idx % AC) * 4;  // rows beyond M repeat the last one; never stored
  }
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int idx = tid + i * 256;
    const int t = idx / WC;
    int row;
    if constexpr (EPI == RE_SWIGLU) row = ((t >> 5) & 1) * g.N + min(n0 + (t >> 6) * 32 + (t & 31), g.N - 1);
    else row = min(n0 + t, g.N - 1);
    wsrc[i] = g.W + (size_t)row * g.K + (idx % WC) * 8;
  }
  f32x4_t aR[NA];
  u32x4_t wR[NW];
  auto stage_load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) aR[i] = *reinterpret_cast<const f32x4_t*>(asrc[i] + k0);
#pragma unroll
    for (int i = 0; i < NW; ++i) wR[i] = *reinterpret_cast<const u32x4_t*>(wsrc[i] + k0);
  };
  auto stage_write = [&]() {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = tid + i * 256;
      const int o = (idx / AC) * RPITCH + (idx % AC) * 4;
      h4_t hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float c = fminf(fmaxf(aR[i][e], -65504.f), 65504.f);
        if (aR[i][e] != aR[i][e]) c = aR[i][e];  // fminf / fmaxf drop a NaN: keep it, so the step's non-finite stop sees it
        hi[e] = (_Float16)c;
        lo[e] = (_Float16)(c - (float)hi[e]);
      }
      *reinterpret_cast<uint2*>(Ah + o) = __builtin_bit_cast(uint2, hi);
      *reinterpret_cast<uint2*>(Al + o) = __builtin_bit_cast(uint2, lo);
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int idx = tid + i * 256;
      *reinterpret_cast<u32x4_t*>(Ws + (idx / WC) * RPITCH + (idx % WC) * 8) = wR[i];
    }
  };

  const int nkt = g.K / RBK;
  stage_load(0);
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();  // every wave is done with the previous k-tile
    stage_write();
    __syncthreads();
    stage_load(min(kt + 1, nkt - 1) * RBK);
#pragma unroll
    for (int kk = 0; kk < RBK; kk += 16) {
      const h8_t ahi = *reinterpret_cast<const h8_t*>(Ah + (wm * 32 + l31) * RPITCH + kk + lh * 8);
      const h8_t alo = *reinterpret_cast<const h8_t*>(Al + (wm * 32 + l31) * RPITCH + kk + lh * 8);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const h8_t b = *reinterpret_cast<const h8_t*>(Ws + (wn * 64 + j * 32 + l31) * RPITCH + kk + lh * 8);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, b, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, b, acc[j], 0, 0, 0);
      }
    }
  }
  // ---- epilogue (C layout: col = lane & 31 -> n, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> m)
  if constexpr (EPI == RE_SWIGLU) {
    const int o = n0 + wn * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const float gt = acc[0][r], up = acc[1][r];
      if (m < g.M && o < g.N) g.out[(size_t)m * g.N + o] = gt / (1.f + expf(-gt)) * up;
    }
  } else {
    // loads first, all of them, indices clamped; only the stores are predicated
    float old[2][16];
    if constexpr (EPI == RE_ADD) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = min(m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, g.M - 1);
          old[j][r] = g.out[(size_t)m * g.N + min(n0 + wn * 64 + j * 32 + l31, g.N - 1)];
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m >= g.M || n >= g.N) continue;
        if constexpr (EPI == RE_ADD) g.out[(size_t)m * g.N + n] = old[j][r] + acc[j][r];
        else g.out[(size_t)m * g.N + n] = acc[j][r];
      }
    }
  }
}

// q_norm / k_norm + RoPE at the row's position, K/V appended to the row's slot cache: grid (M, heads + kv_heads), one wave each
struct RowsAttnP {
  RowsP r;
  const float* qkv;  // [M][heads*HDIM | kv_heads*HDIM | kv_heads*HDIM]
  const float *qn, *kn, *cosb, *sinb;
  float *kc[MAXS], *vc[MAXS];  // this layer's cache of each slot
  float* qb;   // [M][heads][HDIM]
  float* att;  // [M][heads][HDIM]
  int heads, kv_heads, smax;
  float eps, scale;
};

__global__ __launch_bounds__(64) void qrows_prep_kernel(RowsAttnP p) {
  const int row = blockIdx.x, hh = blockIdx.y, lane = threadIdx.x;
  const int slot = p.r.row_slot[row], pos = p.r.row_pos[row];
  const float* cs = p.cosb + (size_t)pos * (HDIM / 2);
  const float* sn = p.sinb + (size_t)pos * (HDIM / 2);
  const int qdim = p.heads * HDIM, kvdim = p.kv_heads * HDIM;
  const float* x = p.qkv + (size_t)row * (qdim + 2 * kvdim);
  if (hh < p.heads) {
    norm_rope_head(x + (size_t)hh * HDIM, p.qn, cs, sn, p.eps, true, lane, p.qb + ((size_t)row * p.heads + hh) * HDIM);
  } else {
    const int kvh = hh - p.heads;
    norm_rope_head(x + qdim + (size_t)kvh * HDIM, p.kn, cs, sn, p.eps, true, lane, pick_slot(p.kc, slot) + ((size_t)kvh * p.smax + pos) * HDIM);
    const float* v = x + qdim + kvdim + (size_t)kvh * HDIM;
    float* vd = pick_slot(p.vc, slot) + ((size_t)kvh * p.smax + pos) * HDIM;
    vd[lane] = v[lane];
    vd[lane + 64] = v[lane + 64];
  }
}

// causal attention of the rows, grid (kv_heads, M): row (s, pos) and its NREP query heads over keys 0..pos of slot s (fp32,
// the lane layout and the online softmax of qattn_kernel; the 16 lane groups are merged and normalised here)
template <int NREP>
__global__ __launch_bounds__(256) void qrows_attn_kernel(RowsAttnP p) {
  __shared__ float gm[16][NREP], gl[16][NREP];
  __shared__ __attribute__((aligned(16))) float gacc[16][NREP][HDIM];
  const int kvh = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
  const int slot = p.r.row_slot[row], pos = p.r.row_pos[row];
  const int g = tid >> 4, dl = tid & 15;
  float q[NREP][8], m[NREP], l[NREP], acc[NREP][8];
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    const float* qp = p.qb + ((size_t)row * p.heads + kvh * NREP + j) * HDIM + dl * 8;
    m[j] = -INFINITY, l[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) q[j][i] = qp[i], acc[j][i] = 0.f;
  }
  const float* kb = pick_slot(p.kc, slot) + (size_t)kvh * p.smax * HDIM + dl * 8;
  const float* vb = pick_slot(p.vc, slot) + (size_t)kvh * p.smax * HDIM + dl * 8;
  for (int key = g; key <= pos; key += 16) {
    const float4 k0 = *reinterpret_cast<const float4*>(kb + (size_t)key * HDIM);
    const float4 k1 = *reinterpret_cast<const float4*>(kb + (size_t)key * HDIM + 4);
    const float4 v0 = *reinterpret_cast<const float4*>(vb + (size_t)key * HDIM);
    const float4 v1 = *reinterpret_cast<const float4*>(vb + (size_t)key * HDIM + 4);
    const float kv[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
    const float vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) d = fmaf(q[j][i], kv[i], d);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) d += __shfl_xor(d, o, 64);
      const float sc = d * p.scale;
      const float mn = fmaxf(m[j], sc);
      const float a = expf(m[j] - mn), e = expf(sc - mn);
      l[j] = fmaf(l[j], a, e);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j][i] = fmaf(acc[j][i], a, e * vv[i]);
      m[j] = mn;
    }
  }
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    if (dl == 0) gm[g][j] = m[j], gl[g][j] = l[j];
#pragma unroll
    for (int i = 0; i < 8; ++i) gacc[g][j][dl * 8 + i] = acc[j][i];
  }
  __syncthreads();
  for (int t = tid; t < NREP * HDIM; t += 256) {
    const int j = t / HDIM, d = t % HDIM;
    float M = -INFINITY;
#pragma unroll
    for (int gg = 0; gg < 16; ++gg) M = fmaxf(M, gm[gg][j]);
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int gg = 0; gg < 16; ++gg) {
      const float e = gm[gg][j] == -INFINITY ? 0.f : expf(gm[gg][j] - M);  // key 0 always exists: M is finite
      o = fmaf(e, gacc[gg][j][d], o);
      L = fmaf(e, gl[gg][j], L);
    }
    p.att[((size_t)row * p.heads + kvh * NREP + j) * HDIM + d] = o / L;
  }
}

// ---- token selection
// order: larger value first, then the lower id (the argmax tie rule of this project)
__device__ __forceinline__ bool before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// bitonic sort of n (a power of two) pairs in LDS into that order
__device__ void bitonic_sort(float* v, int* id, int n) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int o = i ^ j;
        if (o > i) {
          const float a = v[i], b = v[o];
          const int ia = id[i], ib = id[o];
          const bool first = before(a, ia, b, ib);
          if (((i & k) == 0) != first) {
            v[i] = b, v[o] = a, id[i] = ib, id[o] = ia;
          }
        }
      }
      __syncthreads();
    }
}

// pass 1, grid (SAMP_WG, slots): workgroup b takes logits [b*chunk, (b+1)*chunk) of its slot and writes its best kc (value, id) pairs in order
__global__ __launch_bounds__(256) void qsamp_a_kernel(const float* logits, int V, int chunk, const SampDev* sd, float* cv, int* ci) {
  __shared__ float v[SAMP_CHUNK];
  __shared__ int id[SAMP_CHUNK];
  const int kc = sd->kc;
  logits += (size_t)blockIdx.y * V, cv += (size_t)blockIdx.y * SAMP_WG * KC_MAX, ci += (size_t)blockIdx.y * SAMP_WG * KC_MAX;  // this slot's
  const int b = blockIdx.x, tid = threadIdx.x;
  const int beg = b * chunk, end = min(V, beg + chunk);
  if (kc == 1) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = beg + tid; i < end; i += 256) {
      const float x = logits[i];
      if (before(x, i, bv, bi)) bv = x, bi = i;
    }
    v[tid] = bv, id[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s && before(v[tid + s], id[tid + s], v[tid], id[tid])) v[tid] = v[tid + s], id[tid] = id[tid + s];
      __syncthreads();
    }
    if (tid == 0) cv[b * KC_MAX] = v[0], ci[b * KC_MAX] = id[0];
    return;
  }
  int np = kc;  // a power of two, like the padded chunk
  while (np < chunk) np <<= 1;
  for (int i = tid; i < np; i += 256) {
    const int gi = beg + i;
    const bool in = i < chunk && gi < end;
    v[i] = in ? logits[gi] : -INFINITY;
    id[i] = in ? gi : 0x7fffffff;
  }
  __syncthreads();
  bitonic_sort(v, id, np);
  for (int i = tid; i < kc; i += 256) cv[b * KC_MAX + i] = v[i], ci[b * KC_MAX + i] = id[i];
}

struct SeqDev {  // slot 0's; slot z is z * tstride tokens, z ints and z * KC_MAX kept entries further on
  int32_t* tokens;  // [max_seq + 1]: prompt, then generated
  int* cur_len;     // position the next step forwards
  int* gen_count;
  int* finished;
  const int* eos;   // [n_eos]
  int n_eos, smax, V;
  int32_t* kept_id;  // [KC_MAX]
  float* kept_p;
  int* n_kept;
  int tstride;
};

__device__ __forceinline__ int pick(const int32_t* ids, const float* pr, int n, float u) {
  float c = 0.f;
  for (int i = 0; i < n; ++i) {
    c += pr[i];
    if (u < c) return ids[i];
  }
  return ids[n - 1];
}

// pass 2 (one workgroup per slot): the best top_k of the candidates, temperature, top-p, the draw; moves the sequence
__global__ __launch_bounds__(1024) void qsamp_b_kernel(const float* cv, const int* ci, const SampDev* sd, SeqDev s) {
  __shared__ float v[SAMP_WG * KC_MAX];
  __shared__ int id[SAMP_WG * KC_MAX];
  __shared__ float e[KC_MAX];
  const int kc = sd->kc, tid = threadIdx.x, z = blockIdx.x;
  cv += (size_t)z * SAMP_WG * KC_MAX, ci += (size_t)z * SAMP_WG * KC_MAX;
  s.tokens += (size_t)z * s.tstride, s.cur_len += z, s.gen_count += z, s.finished += z, s.n_kept += z;
  s.kept_id += z * KC_MAX, s.kept_p += z * KC_MAX;
  if (*s.finished) return;  // block-uniform
  const int n = SAMP_WG * kc;  // a power of two
  for (int i = tid; i < n; i += 1024) {
    const int b = i / kc, j = i % kc;
    v[i] = cv[b * KC_MAX + j];
    id[i] = ci[b * KC_MAX + j];
  }
  __syncthreads();
  bitonic_sort(v, id, n);
  if (tid != 0) return;
  const int pos = *s.cur_len, gen = *s.gen_count;
  int tok, nk;
  if (!sd->do_sample) {
    tok = id[0];
    nk = 1;
    s.kept_id[0] = tok, s.kept_p[0] = 1.f;
  } else {
    const int k = sd->top_k;
    const float T = sd->temperature;
    const float s0 = v[0] / T;
    float Z = 0.f;
    for (int i = 0; i < k; ++i) {
      e[i] = expf(v[i] / T - s0);
      Z += e[i];
    }
    // TopPLogitsWarper: ascending cumulative probabilities; drop those <= 1 - top_p, never the most likely
    nk = k;
    if (sd->top_p < 1.f) {
      float c = 0.f;
      for (int i = k - 1; i >= 1; --i) {
        c += e[i] / Z;
        if (c <= 1.f - sd->top_p) nk = i;
        else break;
      }
    }
    float Zk = 0.f;
    for (int i = 0; i < nk; ++i) Zk += e[i];
    for (int i = 0; i < nk; ++i) s.kept_id[i] = id[i], s.kept_p[i] = e[i] / Zk;
    tok = pick(s.kept_id, s.kept_p, nk, uniform01(sd->seed, 0u, (unsigned int)gen));
  }
  *s.n_kept = nk;
  if (tok < 0 || tok >= s.V) {
    // only non-finite logits leave no real candidate: the sequence stops with the error mark, no token is emitted
    *s.finished = 3;
    return;
  }
  s.tokens[pos + 1] = tok;
  *s.gen_count = gen + 1;
  bool eos = false;
  for (int i = 0; i < s.n_eos; ++i) eos |= tok == s.eos[i];
  if (pos + 1 < s.smax) *s.cur_len = pos + 1;  // an EOS position is forwarded again by later steps: harmless, no new token
  *s.finished = eos ? 1 : (pos + 1 >= s.smax ? 2 : 0);
}

__global__ void qdraw_kernel(const int32_t* kept_id, const float* kept_p, const int* n_kept, unsigned long long seed, int n, int32_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = pick(kept_id, kept_p, *n_kept, uniform01(seed, 0u, (unsigned int)i));
}

// fp32 host data -> the weight dtype (matrices) or fp32 rounded through it (vectors)
template <typename WT>
__global__ void qconvert_kernel(const float* src, WT* dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = (WT)src[i];
}
__global__ void qround_f16_kernel(const float* src, float* dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = (float)(_Float16)src[i];
}

struct TD {
  size_t off;      // byte offset of the tensor's first row in the arena
  int64_t d0, d1;  // [d0] or [d0][d1]
  bool mat, set = false;
};

struct LW {
  size_t wqkv, wo, wgu, wd, ln1, ln2, qn, kn;
};

}  // namespace qw
}  // namespace ixtts

using namespace ixtts;
using namespace ixtts::qw;

struct ixtts_qwen {
  ixtts_qwen_cfg cfg;
  int D, L, H, KVH, I, V, smax, nrep;
  bool f16;
  size_t esz;
  uint8_t* arena = nullptr;
  size_t arena_bytes = 0;
  std::vector<LW> lw;
  size_t emb = 0, lmh = 0, fnorm = 0;
  bool finalized = false;
  std::map<std::string, TD> tens;
  float *h = nullptr, *qkv = nullptr, *part = nullptr, *ff = nullptr, *logits = nullptr, *kc = nullptr, *vc = nullptr;
  float *cosb = nullptr, *sinb = nullptr, *cv = nullptr, *kept_p = nullptr, *tmp = nullptr;
  size_t tmp_floats = 0;
  int *ci = nullptr, *cur_len = nullptr, *gen_count = nullptr, *finished = nullptr, *n_kept = nullptr, *eos = nullptr;
  int32_t *tokens = nullptr, *kept_id = nullptr, *draws = nullptr;
  int draws_cap = 0;
  SampDev* d_samp = nullptr;
  SampDev samp_host;
  hipStream_t cap_stream = nullptr;
  // [0] one step, [1] STEPS_PER_GRAPH steps; pre / chunk per slot (f32 engines prefill slot after slot), slots_exec[n - 2]
  hipGraphExec_t full_exec[2] = {}, pre_exec[MAXS][2] = {}, chunk_exec[MAXS][2] = {}, slots_exec[MAXS - 1][2] = {};
  float* qb = nullptr;  // [PCH][heads][HDIM]
  // slots: tokens, cur_len, gen_count, finished, n_kept, kept_*, logits, cv / ci hold MAXS entries from create on (slot 0
  // first); the K/V caches of slots 1.. and the buffers of the rows prefill come with the first batched call
  int n_slots = 1, rows_max = 1024;
  int plen[MAXS] = {};  // prompt length per slot
  float *kcs[MAXS] = {}, *vcs[MAXS] = {};
  float *rx = nullptr, *rxn = nullptr, *rqkv = nullptr, *rqb = nullptr, *ratt = nullptr, *rff = nullptr;
  int *row_slot = nullptr, *row_pos = nullptr;
  int tstride() const { return smax + 1; }
};

#define Q_ARENA(off) reinterpret_cast<void*>(h->arena + (off))

static int q_launch_gemv(ixtts_qwen* h, int pro, int epi, GemvP p, hipStream_t st, int nc = 1, int nact = 0) {
  p.tstride = h->tstride();
  p.nact = nact ? nact : nc;
  const int rows = p.N > 16384 && nc == 1 ? 4 : 2;
  const int outs = epi == EPI_SWIGLU ? rows / 2 : rows;
  const int units = (p.N + outs - 1) / outs;
  const dim3 grid((units + WAVES - 1) / WAVES), block(64 * WAVES);
  const size_t lds = (size_t)nc * p.K * sizeof(float);
#define Q_GEMV(WT, PRO, EPI)                                                                            \
  do {                                                                                                  \
    if (nc == PCH) hipLaunchKernelGGL((qgemv_kernel<WT, PRO, EPI, 2, PCH>), grid, block, lds, st, p);  \
    else if (nc == 2) hipLaunchKernelGGL((qgemv_kernel<WT, PRO, EPI, 2, 2>), grid, block, lds, st, p); \
    else if (rows == 4) hipLaunchKernelGGL((qgemv_kernel<WT, PRO, EPI, 4, 1>), grid, block, lds, st, p); \
    else hipLaunchKernelGGL((qgemv_kernel<WT, PRO, EPI, 2, 1>), grid, block, lds, st, p);              \
  } while (0)
#define Q_GEMV_DT(PRO, EPI)                  \
  do {                                       \
    if (h->f16) Q_GEMV(_Float16, PRO, EPI);  \
    else Q_GEMV(float, PRO, EPI);            \
  } while (0)
  if (pro == PRO_EMBED && epi == EPI_STORE) Q_GEMV_DT(PRO_EMBED, EPI_STORE);
  else if (pro == PRO_NORM && epi == EPI_STORE) Q_GEMV_DT(PRO_NORM, EPI_STORE);
  else if (pro == PRO_MERGE && epi == EPI_ADD) Q_GEMV_DT(PRO_MERGE, EPI_ADD);
  else if (pro == PRO_NORM && epi == EPI_SWIGLU) Q_GEMV_DT(PRO_NORM, EPI_SWIGLU);
  else if (pro == PRO_PLAIN && epi == EPI_ADD) Q_GEMV_DT(PRO_PLAIN, EPI_ADD);
  else {
    set_error("qwen: no GEMV variant %d/%d", pro, epi);
    return IXTTS_ERR_ARG;
  }
#undef Q_GEMV_DT
#undef Q_GEMV
  return IXTTS_OK;
}

enum { STEP_PRE = 0, STEP_FULL = 1, STEP_CHUNK = 2, STEP_SLOTS = 3 };

// STEP_PRE: one prompt position through the layers, the position moves on; STEP_FULL: the same, then norm + lm_head + token
// selection; STEP_CHUNK: PCH prompt positions through the layers with one pass over the weights, the position moves PCH on.
// These three act on slot `arg`.  STEP_SLOTS: one decode step (as STEP_FULL) of slots 0..arg-1, column c = slot c; the
// GEMVs are built 2 and PCH columns wide, so a step of 3 slots carries an idle 4th column: it reads slot 3's (valid) token
// and stores nothing (GemvP::nact), and it has no attention and no token selection: slot 3 is left as it is, logits included.
static int q_issue_step(ixtts_qwen* h, int mode, hipStream_t st, int arg = 0) {
  const int D = h->D, qd = h->H * HDIM, kvd = h->KVH * HDIM;
  const float eps = h->cfg.rms_norm_eps;
  const bool slots = mode == STEP_SLOTS;
  const bool full = mode == STEP_FULL || slots;
  const int nc = mode == STEP_CHUNK ? PCH : slots ? (arg <= 2 ? 2 : PCH) : 1;
  const int ns = slots ? arg : 1, s0 = slots ? 0 : arg;
  const int nact = slots ? ns : nc;
  int32_t* const tokens = h->tokens + (size_t)s0 * h->tstride();
  int* const cur_len = h->cur_len + s0;
  for (int l = 0; l < h->L; ++l) {
    const LW& w = h->lw[l];
    GemvP a = {};
    a.w = Q_ARENA(w.wqkv), a.N = qd + 2 * kvd, a.K = D, a.x = h->h, a.g = (const float*)Q_ARENA(w.ln1), a.eps = eps, a.out = h->qkv;
    a.emb = Q_ARENA(h->emb), a.tokens = tokens, a.cur_len = cur_len, a.h_out = h->h, a.slots = slots;
    IX_TRY(q_launch_gemv(h, l == 0 ? PRO_EMBED : PRO_NORM, EPI_STORE, a, st, nc, nact));
    AttnP at;
    at.qkv = h->qkv, at.qn = (const float*)Q_ARENA(w.qn), at.kn = (const float*)Q_ARENA(w.kn), at.cosb = h->cosb, at.sinb = h->sinb;
    for (int z = 0; z < MAXS; ++z) {
      const int sl = std::min(s0 + z, h->n_slots - 1);
      at.kc[z] = h->kcs[sl] ? h->kcs[sl] + (size_t)l * h->KVH * h->smax * HDIM : nullptr;
      at.vc[z] = h->vcs[sl] ? h->vcs[sl] + (size_t)l * h->KVH * h->smax * HDIM : nullptr;
    }
    at.cur_len = cur_len, at.finished = slots ? h->finished : nullptr, at.part = h->part, at.heads = h->H, at.kv_heads = h->KVH, at.smax = h->smax, at.eps = eps;
    at.scale = 1.f / sqrtf((float)HDIM), at.qb = h->qb;
    const dim3 ag(h->KVH, NSP, ns);
    if (mode == STEP_CHUNK) {
      hipLaunchKernelGGL(qprep_kernel, dim3(PCH, h->H + h->KVH), dim3(64), 0, st, at);
      if (h->nrep == 1) hipLaunchKernelGGL(qattn_chunk_kernel<1>, ag, dim3(256), 0, st, at);
      else if (h->nrep == 2) hipLaunchKernelGGL(qattn_chunk_kernel<2>, ag, dim3(256), 0, st, at);
      else hipLaunchKernelGGL(qattn_chunk_kernel<4>, ag, dim3(256), 0, st, at);
    } else if (h->nrep == 1) hipLaunchKernelGGL(qattn_kernel<1>, ag, dim3(256), 0, st, at);
    else if (h->nrep == 2) hipLaunchKernelGGL(qattn_kernel<2>, ag, dim3(256), 0, st, at);
    else hipLaunchKernelGGL(qattn_kernel<4>, ag, dim3(256), 0, st, at);
    GemvP o = {};
    o.w = Q_ARENA(w.wo), o.N = D, o.K = qd, o.out = h->h, o.part = h->part;
    IX_TRY(q_launch_gemv(h, PRO_MERGE, EPI_ADD, o, st, nc, nact));
    GemvP gu = {};
    gu.w = Q_ARENA(w.wgu), gu.N = h->I, gu.K = D, gu.x = h->h, gu.g = (const float*)Q_ARENA(w.ln2), gu.eps = eps, gu.out = h->ff;
    IX_TRY(q_launch_gemv(h, PRO_NORM, EPI_SWIGLU, gu, st, nc, nact));
    GemvP dn = {};
    dn.w = Q_ARENA(w.wd), dn.N = D, dn.K = h->I, dn.x = h->ff, dn.out = h->h;
    dn.advance = (!full && l == h->L - 1) ? cur_len : nullptr;
    IX_TRY(q_launch_gemv(h, PRO_PLAIN, EPI_ADD, dn, st, nc, nact));
  }
  if (full) {
    GemvP hd = {};
    hd.w = Q_ARENA(h->lmh), hd.N = h->V, hd.K = D, hd.x = h->h, hd.g = (const float*)Q_ARENA(h->fnorm), hd.eps = eps, hd.out = h->logits;
    IX_TRY(q_launch_gemv(h, PRO_NORM, EPI_STORE, hd, st, nc, nact));
    const int chunk = (h->V + SAMP_WG - 1) / SAMP_WG;
    hipLaunchKernelGGL(qsamp_a_kernel, dim3(SAMP_WG, ns), dim3(256), 0, st, h->logits, h->V, chunk, h->d_samp, h->cv, h->ci);
    SeqDev s{h->tokens, h->cur_len, h->gen_count, h->finished, h->eos, h->cfg.n_eos, h->smax, h->V, h->kept_id, h->kept_p, h->n_kept,
             h->tstride()};
    hipLaunchKernelGGL(qsamp_b_kernel, dim3(ns), dim3(1024), 0, st, h->cv, h->ci, h->d_samp, s);
  }
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

static int q_graph(ixtts_qwen* h, int mode, int reps, hipGraphExec_t* out, int arg) {
  hipGraph_t g;
  hipStream_t cs = h->cap_stream;
  IX_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
  int rc = IXTTS_OK;
  for (int r = 0; r < reps && rc == IXTTS_OK; ++r) rc = q_issue_step(h, mode, cs, arg);
  hipError_t e = hipStreamEndCapture(cs, &g);
  if (rc != IXTTS_OK) return rc;
  IX_HIP(e);
  IX_HIP(hipGraphInstantiate(out, g, nullptr, nullptr, 0));
  IX_HIP(hipGraphDestroy(g));
  return IXTTS_OK;
}

static int q_run(ixtts_qwen* h, int mode, int n, hipStream_t st, int arg = 0) {
  for (int done = 0; done < n;) {
    const int big = n - done >= STEPS_PER_GRAPH ? 1 : 0;
    hipGraphExec_t* slot = mode == STEP_FULL    ? &h->full_exec[big]
                           : mode == STEP_CHUNK ? &h->chunk_exec[arg][big]
                           : mode == STEP_PRE   ? &h->pre_exec[arg][big]
                                                : &h->slots_exec[arg - 2][big];
    if (!*slot) IX_TRY(q_graph(h, mode, big ? STEPS_PER_GRAPH : 1, slot, arg));
    IX_HIP(hipGraphLaunch(*slot, st));
    done += big ? STEPS_PER_GRAPH : 1;
  }
  return IXTTS_OK;
}

#define Q_READY(h, who)                                    \
  do {                                                     \
    IX_ARG(h, who ": null handle");                        \
    if (!(h)->finalized) {                                 \
      ::ixtts::set_error(who ": call ixtts_qwen_finalize"); \
      return IXTTS_ERR_STATE;                              \
    }                                                      \
  } while (0)

static void q_free(ixtts_qwen* h) {
  for (int i = 0; i < 2; ++i) {
    if (h->full_exec[i]) hipGraphExecDestroy(h->full_exec[i]);
    for (int z = 0; z < MAXS; ++z) {
      if (h->pre_exec[z][i]) hipGraphExecDestroy(h->pre_exec[z][i]);
      if (h->chunk_exec[z][i]) hipGraphExecDestroy(h->chunk_exec[z][i]);
      if (z < MAXS - 1 && h->slots_exec[z][i]) hipGraphExecDestroy(h->slots_exec[z][i]);
    }
  }
  void* ptrs[] = {h->arena, h->h, h->qkv, h->part, h->ff, h->logits, h->kc, h->vc, h->cosb, h->sinb, h->cv, h->kept_p, h->tmp, h->qb, h->ci,
                  h->cur_len, h->gen_count, h->finished, h->n_kept, h->eos, h->tokens, h->kept_id, h->draws, h->d_samp,
                  h->rx, h->rxn, h->rqkv, h->rqb, h->ratt, h->rff, h->row_slot, h->row_pos};
  for (void* p : ptrs)
    if (p) hipFree(p);
  for (int z = 1; z < MAXS; ++z) {  // [0] are kc / vc
    if (h->kcs[z]) hipFree(h->kcs[z]);
    if (h->vcs[z]) hipFree(h->vcs[z]);
  }
  if (h->cap_stream) hipStreamDestroy(h->cap_stream);
}

extern "C" int ixtts_qwen_create(ixtts_qwen** out, const ixtts_qwen_cfg* c) { return ixtts_qwen_create_slots(out, c, 1); }

extern "C" int ixtts_qwen_create_slots(ixtts_qwen** out, const ixtts_qwen_cfg* c, int n_slots) {
  IX_ARG(out && c, "qwen_create: null argument");
  *out = nullptr;
  IX_ARG(n_slots >= 1 && n_slots <= MAXS, "qwen_create: %d slots (1..%d)", n_slots, MAXS);
  IX_ARG(c->head_dim == HDIM, "qwen_create: head_dim %d (only %d is built)", c->head_dim, HDIM);
  IX_ARG(c->layers >= 1 && c->heads >= 1 && c->kv_heads >= 1 && c->heads % c->kv_heads == 0, "qwen_create: heads %d / kv_heads %d", c->heads,
         c->kv_heads);
  const int nrep = c->heads / c->kv_heads;
  IX_ARG(nrep == 1 || nrep == 2 || nrep == 4, "qwen_create: heads / kv_heads = %d (built: 1, 2, 4)", nrep);
  IX_ARG(c->hidden_size > 0 && c->hidden_size % 512 == 0 && c->intermediate_size > 0 && c->intermediate_size % 512 == 0 &&
             (c->heads * HDIM) % 512 == 0,
         "qwen_create: hidden_size %d, intermediate_size %d and heads*head_dim must be multiples of 512", c->hidden_size, c->intermediate_size);
  IX_ARG(c->hidden_size <= 16384 && c->intermediate_size <= 16384 && c->heads * HDIM <= 16384, "qwen_create: a GEMV input wider than 16384");
  IX_ARG(c->vocab_size >= SAMP_WG && c->vocab_size <= SAMP_WG * SAMP_CHUNK, "qwen_create: vocab_size %d (built: %d..%d)", c->vocab_size, SAMP_WG,
         SAMP_WG * SAMP_CHUNK);
  IX_ARG(c->max_seq >= 2 && c->max_seq <= (1 << 20), "qwen_create: max_seq %d", c->max_seq);
  IX_ARG(c->weight_dtype == IXTTS_DTYPE_F32 || c->weight_dtype == IXTTS_DTYPE_F16, "qwen_create: weight_dtype %d (f32 or f16)", c->weight_dtype);
  IX_ARG(c->n_eos >= 1 && c->n_eos <= IXTTS_QWEN_MAX_EOS, "qwen_create: n_eos %d", c->n_eos);
  IX_ARG(c->rms_norm_eps > 0.f && c->rope_theta > 0.f, "qwen_create: rms_norm_eps / rope_theta");
  for (int i = 0; i < c->n_eos; ++i) IX_ARG(c->eos_ids[i] >= 0 && c->eos_ids[i] < c->vocab_size, "qwen_create: eos id %d", c->eos_ids[i]);
  ixtts_qwen* h = new ixtts_qwen();
  h->cfg = *c;
  h->D = c->hidden_size, h->L = c->layers, h->H = c->heads, h->KVH = c->kv_heads, h->I = c->intermediate_size, h->V = c->vocab_size;
  h->smax = c->max_seq, h->nrep = nrep, h->f16 = c->weight_dtype == IXTTS_DTYPE_F16;
  h->esz = h->f16 ? 2 : 4;
  h->n_slots = n_slots;
  if (const char* e = getenv("IXTTS_QWEN_ROWS_MAX")) {  // tests: several passes of the rows prefill without long prompts
    const int v = atoi(e);
    if (v < 1 || v > 65536) {
      set_error("qwen_create: IXTTS_QWEN_ROWS_MAX=%s (1..65536)", e);
      delete h;
      return IXTTS_ERR_ARG;
    }
    h->rows_max = v;
  }
  // ---- arena layout: matrices in the weight dtype, vectors fp32; every tensor 256-byte aligned
  size_t off = 0;
  const int D = h->D, qd = h->H * HDIM, kvd = h->KVH * HDIM;
  auto mat = [&](const std::string& name, int64_t rows, int64_t cols) {
    off = align_up(off, 256);
    h->tens[name] = TD{off, rows, cols, true};
    const size_t o = off;
    off += (size_t)rows * cols * h->esz;
    return o;
  };
  auto sub = [&](const std::string& name, size_t base, int64_t row0, int64_t rows, int64_t cols) {
    h->tens[name] = TD{base + (size_t)row0 * cols * h->esz, rows, cols, true};
  };
  auto vec = [&](const std::string& name, int64_t n) {
    off = align_up(off, 256);
    h->tens[name] = TD{off, n, 0, false};
    const size_t o = off;
    off += (size_t)n * 4;
    return o;
  };
  h->emb = mat("model.embed_tokens.weight", h->V, D);
  h->lw.resize(h->L);
  for (int l = 0; l < h->L; ++l) {
    const std::string p = "model.layers." + std::to_string(l) + ".";
    LW& w = h->lw[l];
    w.wqkv = mat(p + "qkv", qd + 2 * kvd, D);
    sub(p + "self_attn.q_proj.weight", w.wqkv, 0, qd, D);
    sub(p + "self_attn.k_proj.weight", w.wqkv, qd, kvd, D);
    sub(p + "self_attn.v_proj.weight", w.wqkv, qd + kvd, kvd, D);
    h->tens.erase(p + "qkv");
    w.wo = mat(p + "self_attn.o_proj.weight", D, qd);
    w.wgu = mat(p + "gu", 2 * (int64_t)h->I, D);
    sub(p + "mlp.gate_proj.weight", w.wgu, 0, h->I, D);
    sub(p + "mlp.up_proj.weight", w.wgu, h->I, h->I, D);
    h->tens.erase(p + "gu");
    w.wd = mat(p + "mlp.down_proj.weight", D, h->I);
    w.ln1 = vec(p + "input_layernorm.weight", D);
    w.ln2 = vec(p + "post_attention_layernorm.weight", D);
    w.qn = vec(p + "self_attn.q_norm.weight", HDIM);
    w.kn = vec(p + "self_attn.k_norm.weight", HDIM);
  }
  h->fnorm = vec("model.norm.weight", D);
  h->lmh = c->tie_word_embeddings ? h->emb : mat("lm_head.weight", h->V, D);
  h->arena_bytes = align_up(off, 256);
  // ---- state
  const size_t kv = (size_t)h->L * h->KVH * h->smax * HDIM;
  int rc = IXTTS_OK;
  auto al = [&](void** p, size_t bytes) {
    if (rc == IXTTS_OK && hipMalloc(p, std::max<size_t>(bytes, 256)) != hipSuccess) {
      set_error("qwen_create: hipMalloc of %zu bytes failed", bytes);
      rc = IXTTS_ERR_NOMEM;
    }
  };
  al((void**)&h->arena, h->arena_bytes);
  al((void**)&h->h, (size_t)PCH * D * 4);
  al((void**)&h->qkv, (size_t)PCH * (qd + 2 * kvd) * 4);
  al((void**)&h->part, (size_t)PCH * h->H * NSP * PSTR * 4);
  al((void**)&h->ff, (size_t)PCH * h->I * 4);
  al((void**)&h->qb, (size_t)PCH * qd * 4);
  al((void**)&h->logits, (size_t)MAXS * h->V * 4);
  al((void**)&h->kc, kv * 4);
  al((void**)&h->vc, kv * 4);
  al((void**)&h->cosb, (size_t)h->smax * (HDIM / 2) * 4);
  al((void**)&h->sinb, (size_t)h->smax * (HDIM / 2) * 4);
  al((void**)&h->cv, (size_t)MAXS * SAMP_WG * KC_MAX * 4);
  al((void**)&h->ci, (size_t)MAXS * SAMP_WG * KC_MAX * 4);
  al((void**)&h->kept_id, (size_t)MAXS * KC_MAX * 4);
  al((void**)&h->kept_p, (size_t)MAXS * KC_MAX * 4);
  al((void**)&h->tokens, (size_t)MAXS * (h->smax + 1) * 4);
  al((void**)&h->cur_len, MAXS * 4);
  al((void**)&h->gen_count, MAXS * 4);
  al((void**)&h->finished, MAXS * 4);
  al((void**)&h->n_kept, MAXS * 4);
  h->kcs[0] = h->kc, h->vcs[0] = h->vc;
  al((void**)&h->eos, (size_t)IXTTS_QWEN_MAX_EOS * 4);
  al((void**)&h->d_samp, sizeof(SampDev));
  if (rc == IXTTS_OK && (hipMemset(h->kc, 0, kv * 4) != hipSuccess || hipMemset(h->vc, 0, kv * 4) != hipSuccess ||
                         hipMemset(h->tokens, 0, (size_t)MAXS * (h->smax + 1) * 4) != hipSuccess ||
                         hipMemset(h->cur_len, 0, MAXS * 4) != hipSuccess || hipMemset(h->gen_count, 0, MAXS * 4) != hipSuccess ||
                         hipMemset(h->n_kept, 0, MAXS * 4) != hipSuccess || hipMemset(h->logits, 0, (size_t)MAXS * h->V * 4) != hipSuccess ||
                         hipMemcpy(h->eos, c->eos_ids, (size_t)c->n_eos * 4, hipMemcpyHostToDevice) != hipSuccess ||
                         hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking) != hipSuccess)) {
    set_error("qwen_create: device initialisation failed");
    rc = IXTTS_ERR_HIP;
  }
  if (rc == IXTTS_OK) {
    // finished = 1 until a prefill: a step before it changes nothing
    const int one[MAXS] = {1, 1, 1, 1};
    if (hipMemcpy(h->finished, one, sizeof(one), hipMemcpyHostToDevice) != hipSuccess) rc = IXTTS_ERR_HIP;
  }
  if (rc == IXTTS_OK) {
    // RoPE tables as HF builds them: inv_freq = 1 / theta^(2i/d) in fp32, angle = fp32(pos * inv_freq), cos/sin of it
    std::vector<float> cs((size_t)h->smax * (HDIM / 2)), sn(cs.size());
    for (int i = 0; i < HDIM / 2; ++i) {
      const float inv = 1.0f / powf(c->rope_theta, (float)(2 * i) / (float)HDIM);
      for (int p = 0; p < h->smax; ++p) {
        const float a = (float)p * inv;
        cs[(size_t)p * (HDIM / 2) + i] = (float)std::cos((double)a);
        sn[(size_t)p * (HDIM / 2) + i] = (float)std::sin((double)a);
      }
    }
    if (hipMemcpy(h->cosb, cs.data(), cs.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->sinb, sn.data(), sn.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
      set_error("qwen_create: RoPE table upload failed");
      rc = IXTTS_ERR_HIP;
    }
  }
  if (rc != IXTTS_OK) {
    q_free(h);
    delete h;
    return rc;
  }
  *out = h;
  return IXTTS_OK;
}

extern "C" int ixtts_qwen_set_tensor(ixtts_qwen* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  IX_ARG(h && name && data && shape, "qwen_set_tensor: null argument");
  auto it = h->tens.find(name);
  if (it == h->tens.end()) {
    set_error("qwen_set_tensor: unknown tensor %s", name);
    return IXTTS_ERR_NAME;
  }
  TD& t = it->second;
  const bool okshape = t.mat ? (ndim == 2 && shape[0] == t.d0 && shape[1] == t.d1) : (ndim == 1 && shape[0] == t.d0);
  IX_ARG(okshape, "qwen_set_tensor: %s has the wrong shape", name);
  const size_t n = (size_t)t.d0 * (t.mat ? t.d1 : 1);
  if (h->tmp_floats < n) {
    if (h->tmp) hipFree(h->tmp);
    h->tmp = nullptr;
    if (hipMalloc(&h->tmp, n * 4) != hipSuccess) {
      h->tmp_floats = 0;
      set_error("qwen_set_tensor: hipMalloc of %zu bytes failed", n * 4);
      return IXTTS_ERR_NOMEM;
    }
    h->tmp_floats = n;
  }
  IX_HIP(hipMemcpy(h->tmp, data, n * 4, hipMemcpyHostToDevice));
  const dim3 g((unsigned)std::min<size_t>((n + 255) / 256, 8192)), b(256);
  if (t.mat && h->f16) hipLaunchKernelGGL(qconvert_kernel<_Float16>, g, b, 0, nullptr, h->tmp, (_Float16*)Q_ARENA(t.off), n);
  else if (!t.mat && h->f16) hipLaunchKernelGGL(qround_f16_kernel, g, b, 0, nullptr, h->tmp, (float*)Q_ARENA(t.off), n);
  else hipLaunchKernelGGL(qconvert_kernel<float>, g, b, 0, nullptr, h->tmp, (float*)Q_ARENA(t.off), n);
  IX_HIP(hipGetLastError());
  IX_HIP(hipDeviceSynchronize());
  t.set = true;
  return IXTTS_OK;
}

extern "C" int ixtts_qwen_finalize(ixtts_qwen* h) {
  IX_ARG(h, "qwen_finalize: null handle");
  for (auto& kv : h->tens) IX_ARG(kv.second.set, "qwen_finalize: tensor %s was never set", kv.first.c_str());
  if (h->tmp) hipFree(h->tmp);
  h->tmp = nullptr, h->tmp_floats = 0;
  h->finalized = true;
  return IXTTS_OK;
}

static int q_set_sampling(ixtts_qwen* h, const ixtts_qwen_sampling* sc, hipStream_t st) {
  IX_ARG(sc, "qwen: null sampling");
  SampDev d;
  d.do_sample = sc->do_sample ? 1 : 0;
  d.temperature = sc->temperature, d.top_p = sc->top_p, d.top_k = sc->top_k, d.seed = sc->seed;
  if (d.do_sample) {
    IX_ARG(sc->temperature > 0.f, "qwen: temperature %g must be positive", (double)sc->temperature);
    IX_ARG(sc->top_p > 0.f && sc->top_p <= 1.f, "qwen: top_p %g outside (0, 1]", (double)sc->top_p);
    IX_ARG(sc->top_k >= 1 && sc->top_k <= KC_MAX, "qwen: top_k %d outside 1..%d (the device top-k limit)", sc->top_k, KC_MAX);
    d.top_k = std::min(sc->top_k, h->V);
    int kc = 1;
    while (kc < d.top_k) kc <<= 1;
    d.kc = kc;
  } else {
    d.top_k = 1, d.kc = 1;
  }
  h->samp_host = d;
  IX_HIP(hipMemcpyAsync(h->d_samp, &h->samp_host, sizeof(SampDev), hipMemcpyHostToDevice, st));
  return IXTTS_OK;
}

extern "C" int ixtts_qwen_prefill(ixtts_qwen* h, const int32_t* ids, int n, void* stream) {
  Q_READY(h, "qwen_prefill");
  IX_ARG(ids, "qwen_prefill: null ids");
  IX_ARG(n >= 1 && n < h->smax, "qwen_prefill: %d prompt ids (1..%d)", n, h->smax - 1);
  for (int i = 0; i < n; ++i) IX_ARG(ids[i] >= 0 && ids[i] < h->V, "qwen_prefill: id %d at %d outside the vocabulary", ids[i], i);
  hipStream_t st = (hipStream_t)stream;
  IX_HIP(hipStreamSynchronize(st));  // the previous sequence is done with the token buffer
  IX_HIP(hipMemcpyAsync(h->tokens, ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
  IX_HIP(hipMemsetAsync(h->cur_len, 0, 4, st));
  IX_HIP(hipMemsetAsync(h->gen_count, 0, 4, st));
  IX_HIP(hipMemsetAsync(h->finished, 0, 4, st));
  IX_HIP(hipMemsetAsync(h->n_kept, 0, 4, st));
  IX_HIP(hipStreamSynchronize(st));
  h->plen[0] = n;
  // the first n-1 positions: PCH per weight pass, the rest one by one
  IX_TRY(q_run(h, STEP_CHUNK, (n - 1) / PCH, st));
  IX_TRY(q_run(h, STEP_PRE, (n - 1) % PCH, st));
  return IXTTS_OK;
}

extern "C" int ixtts_qwen_step(ixtts_qwen* h, int n_steps, const ixtts_qwen_sampling* sc, void* stream) {
  Q_READY(h, "qwen_step");
  IX_ARG(n_steps >= 0, "qwen_step: n_steps %d", n_steps);
  IX_ARG(h->plen[0] > 0, "qwen_step: no prompt (call ixtts_qwen_prefill)");
  hipStream_t st = (hipStream_t)stream;
  IX_TRY(q_set_sampling(h, sc, st));
  IX_TRY(q_run(h, STEP_FULL, n_steps, st));
  return IXTTS_OK;
}

#define Q_SLOT(h, slot, who) IX_ARG((slot) >= 0 && (slot) < (h)->n_slots, who ": slot %d of an engine of %d", slot, (h)->n_slots)

extern "C" int ixtts_qwen_read_slot(ixtts_qwen* h, int slot, int32_t* ids, int cap, int* n_ids, int* finished, void* stream) {
  Q_READY(h, "qwen_read");
  Q_SLOT(h, slot, "qwen_read");
  IX_ARG(n_ids && finished && (ids || cap == 0) && cap >= 0, "qwen_read: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  IX_HIP(hipStreamSynchronize(st));
  int g = 0, f = 0;
  IX_HIP(hipMemcpy(&g, h->gen_count + slot, 4, hipMemcpyDeviceToHost));
  IX_HIP(hipMemcpy(&f, h->finished + slot, 4, hipMemcpyDeviceToHost));
  if (f == 3) {
    set_error("qwen_read: the logits of step %d were not finite, no token could be selected", g);
    return IXTTS_ERR_STATE;
  }
  const int m = std::min(g, cap);
  if (m > 0) IX_HIP(hipMemcpy(ids, h->tokens + (size_t)slot * h->tstride() + h->plen[slot], (size_t)m * 4, hipMemcpyDeviceToHost));
  *n_ids = g, *finished = f;
  return IXTTS_OK;
}

extern "C" int ixtts_qwen_read(ixtts_qwen* h, int32_t* ids, int cap, int* n_ids, int* finished, void* stream) {
  return ixtts_qwen_read_slot(h, 0, ids, cap, n_ids, finished, stream);
}

extern "C" int ixtts_qwen_generate(ixtts_qwen* h, int max_new, const ixtts_qwen_sampling* sc, int32_t* ids, int cap, int* n_ids, int* finished,
                                   void* stream) {
  Q_READY(h, "qwen_generate");
  IX_ARG(max_new >= 0, "qwen_generate: max_new %d", max_new);
  IX_ARG(h->plen[0] > 0, "qwen_generate: no prompt (call ixtts_qwen_prefill)");
  hipStream_t st = (hipStream_t)stream;
  IX_TRY(q_set_sampling(h, sc, st));
  // steps past EOS change nothing, so the host only looks every 16 tokens
  max_new = std::min(max_new, h->smax - h->plen[0]);
  int done = 0, g = 0, f = 0;
  while (done < max_new) {
    const int n = std::min(16, max_new - done);
    IX_TRY(q_run(h, STEP_FULL, n, st));
    done += n;
    IX_HIP(hipStreamSynchronize(st));
    IX_HIP(hipMemcpy(&f, h->finished, 4, hipMemcpyDeviceToHost));
    if (f) break;
  }
  IX_TRY(ixtts_qwen_read(h, ids, cap, &g, &f, stream));
  *n_ids = std::min(g, max_new), *finished = f;
  return IXTTS_OK;
}

extern "C" int ixtts_qwen_read_logits_slot(ixtts_qwen* h, int slot, float* out, void* stream) {
  Q_READY(h, "qwen_read_logits");
  Q_SLOT(h, slot, "qwen_read_logits");
  IX_ARG(out, "qwen_read_logits: null output");
  IX_HIP(hipStreamSynchronize((hipStream_t)stream));
  IX_HIP(hipMemcpy(out, h->logits + (size_t)slot * h->V, (size_t)h->V * 4, hipMemcpyDeviceToHost));
  return IXTTS_OK;
}

extern "C" int ixtts_qwen_read_logits(ixtts_qwen* h, float* out, void* stream) { return ixtts_qwen_read_logits_slot(h, 0, out, stream); }

extern "C" int ixtts_qwen_read_kept_slot(ixtts_qwen* h, int slot, int32_t* ids, float* probs, int cap, int* n_kept, void* stream) {
  Q_READY(h, "qwen_read_kept");
  Q_SLOT(h, slot, "qwen_read_kept");
  IX_ARG(ids && probs && n_kept && cap >= 0, "qwen_read_kept: bad arguments");
  IX_HIP(hipStreamSynchronize((hipStream_t)stream));
  int n = 0;
  IX_HIP(hipMemcpy(&n, h->n_kept + slot, 4, hipMemcpyDeviceToHost));
  const int m = std::min(n, cap);
  if (m > 0) {
    IX_HIP(hipMemcpy(ids, h->kept_id + slot * KC_MAX, (size_t)m * 4, hipMemcpyDeviceToHost));
    IX_HIP(hipMemcpy(probs, h->kept_p + slot * KC_MAX, (size_t)m * 4, hipMemcpyDeviceToHost));
  }
  *n_kept = n;
  return IXTTS_OK;
}

extern "C" int ixtts_qwen_read_kept(ixtts_qwen* h, int32_t* ids, float* probs, int cap, int* n_kept, void* stream) {
  return ixtts_qwen_read_kept_slot(h, 0, ids, probs, cap, n_kept, stream);
}

// ---- slots
// the K/V caches of slots 1.. (a batched call of more than one slot needs them)
static int q_slots_ready(ixtts_qwen* h) {
  const size_t kv = (size_t)h->L * h->KVH * h->smax * HDIM * 4;
  for (int z = 1; z < h->n_slots; ++z) {
    if (h->kcs[z] && h->vcs[z]) continue;
    if ((!h->kcs[z] && hipMalloc(&h->kcs[z], kv) != hipSuccess) || (!h->vcs[z] && hipMalloc(&h->vcs[z], kv) != hipSuccess)) {
      (void)hipGetLastError();
      set_error("qwen: hipMalloc of the K/V cache of slot %d (2 x %zu bytes) failed", z, kv);
      return IXTTS_ERR_NOMEM;
    }
    IX_HIP(hipMemset(h->kcs[z], 0, kv));
    IX_HIP(hipMemset(h->vcs[z], 0, kv));
  }
  return IXTTS_OK;
}

static int q_rows_ready(ixtts_qwen* h) {
  const size_t R = h->rows_max, qd = (size_t)h->H * HDIM, kvd = (size_t)h->KVH * HDIM;
  // each buffer only if it is not there yet: a call after a failed one allocates the rest
  auto al = [](auto** p, size_t bytes) {
    if (*p || hipMalloc(p, bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    *p = nullptr;
    set_error("qwen: hipMalloc of %zu bytes for the rows prefill failed", bytes);
    return false;
  };
  const bool ok = al(&h->row_slot, (size_t)MAXS * h->smax * 4) && al(&h->row_pos, (size_t)MAXS * h->smax * 4) && al(&h->rx, R * h->D * 4) &&
                  al(&h->rxn, R * h->D * 4) && al(&h->rqkv, R * (qd + 2 * kvd) * 4) && al(&h->rqb, R * qd * 4) && al(&h->ratt, R * qd * 4) &&
                  al(&h->rff, R * h->I * 4);
  return ok ? IXTTS_OK : IXTTS_ERR_NOMEM;
}

static void q_rows_gemm(int epi, const float* A, const void* W, float* out, int M, int N, int K, hipStream_t st) {
  RGemmP g{A, reinterpret_cast<const _Float16*>(W), out, M, N, K};
  const dim3 grid((N + (epi == RE_SWIGLU ? RBN / 2 : RBN) - 1) / (epi == RE_SWIGLU ? RBN / 2 : RBN), (M + RBM - 1) / RBM), blk(256);
  if (epi == RE_STORE) hipLaunchKernelGGL(qrows_gemm_kernel<RE_STORE>, grid, blk, 0, st, g);
  else if (epi == RE_ADD) hipLaunchKernelGGL(qrows_gemm_kernel<RE_ADD>, grid, blk, 0, st, g);
  else hipLaunchKernelGGL(qrows_gemm_kernel<RE_SWIGLU>, grid, blk, 0, st, g);
}

// the first len - 1 positions of slots 0..n-1 through the layers as rows (f16 engines); cur_len is set by the caller
static int q_prefill_rows(ixtts_qwen* h, int n, const int* lens, hipStream_t st) {
  std::vector<int> rs, rp;
  for (int s = 0; s < n; ++s)
    for (int p = 0; p + 1 < lens[s]; ++p) rs.push_back(s), rp.push_back(p);
  const int total = (int)rs.size();
  if (!total) return IXTTS_OK;
  IX_TRY(q_rows_ready(h));
  IX_HIP(hipMemcpy(h->row_slot, rs.data(), (size_t)total * 4, hipMemcpyHostToDevice));
  IX_HIP(hipMemcpy(h->row_pos, rp.data(), (size_t)total * 4, hipMemcpyHostToDevice));
  const int D = h->D, qd = h->H * HDIM, kvd = h->KVH * HDIM;
  const float eps = h->cfg.rms_norm_eps;
  for (int r0 = 0; r0 < total; r0 += h->rows_max) {
    const int M = std::min(h->rows_max, total - r0);
    const RowsP r{h->row_slot + r0, h->row_pos + r0, M};
    hipLaunchKernelGGL(qrows_embed_kernel, dim3(M), dim3(256), 0, st, r, (const _Float16*)Q_ARENA(h->emb), h->tokens, h->tstride(), D, h->rx);
    for (int l = 0; l < h->L; ++l) {
      const LW& w = h->lw[l];
      hipLaunchKernelGGL(qrows_norm_kernel, dim3(M), dim3(256), 0, st, h->rx, (const float*)Q_ARENA(w.ln1), eps, D, h->rxn);
      q_rows_gemm(RE_STORE, h->rxn, Q_ARENA(w.wqkv), h->rqkv, M, qd + 2 * kvd, D, st);
      RowsAttnP a;
      a.r = r, a.qkv = h->rqkv, a.qn = (const float*)Q_ARENA(w.qn), a.kn = (const float*)Q_ARENA(w.kn), a.cosb = h->cosb, a.sinb = h->sinb;
      for (int z = 0; z < MAXS; ++z) {
        const int sl = std::min(z, n - 1);
        a.kc[z] = h->kcs[sl] + (size_t)l * h->KVH * h->smax * HDIM, a.vc[z] = h->vcs[sl] + (size_t)l * h->KVH * h->smax * HDIM;
      }
      a.qb = h->rqb, a.att = h->ratt, a.heads = h->H, a.kv_heads = h->KVH, a.smax = h->smax, a.eps = eps, a.scale = 1.f / sqrtf((float)HDIM);
      hipLaunchKernelGGL(qrows_prep_kernel, dim3(M, h->H + h->KVH), dim3(64), 0, st, a);
      if (l == h->L - 1) break;  // the last layer's keys and values are all a later step reads of it
      const dim3 ag(h->KVH, M);
      if (h->nrep == 1) hipLaunchKernelGGL(qrows_attn_kernel<1>, ag, dim3(256), 0, st, a);
      else if (h->nrep == 2) hipLaunchKernelGGL(qrows_attn_kernel<2>, ag, dim3(256), 0, st, a);
      else hipLaunchKernelGGL(qrows_attn_kernel<4>, ag, dim3(256), 0, st, a);
      q_rows_gemm(RE_ADD, h->ratt, Q_ARENA(w.wo), h->rx, M, D, qd, st);
      hipLaunchKernelGGL(qrows_norm_kernel, dim3(M), dim3(256), 0, st, h->rx, (const float*)Q_ARENA(w.ln2), eps, D, h->rxn);
      q_rows_gemm(RE_SWIGLU, h->rxn, Q_ARENA(w.wgu), h->rff, M, h->I, D, st);
      q_rows_gemm(RE_ADD, h->rff, Q_ARENA(w.wd), h->rx, M, D, h->I, st);
    }
  }
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

extern "C" int ixtts_qwen_prefill_slots(ixtts_qwen* h, int n, const int32_t* ids, const int* lens, void* stream) {
  Q_READY(h, "qwen_prefill_slots");
  IX_ARG(ids && lens, "qwen_prefill_slots: null argument");
  IX_ARG(n >= 1 && n <= h->n_slots, "qwen_prefill_slots: %d sequences on an engine of %d slots", n, h->n_slots);
  size_t off = 0;
  for (int s = 0; s < n; ++s) {
    IX_ARG(lens[s] >= 1 && lens[s] < h->smax, "qwen_prefill_slots: %d prompt ids in slot %d (1..%d)", lens[s], s, h->smax - 1);
    for (int i = 0; i < lens[s]; ++i)
      IX_ARG(ids[off + i] >= 0 && ids[off + i] < h->V, "qwen_prefill_slots: id %d at %d of slot %d outside the vocabulary", ids[off + i], i, s);
    off += lens[s];
  }
  hipStream_t st = (hipStream_t)stream;
  IX_HIP(hipStreamSynchronize(st));  // the previous sequences are done with the token buffers
  if (n > 1) IX_TRY(q_slots_ready(h));
  int cur[MAXS] = {}, zero[MAXS] = {};
  off = 0;
  for (int s = 0; s < n; ++s) {
    IX_HIP(hipMemcpy(h->tokens + (size_t)s * h->tstride(), ids + off, (size_t)lens[s] * 4, hipMemcpyHostToDevice));
    off += lens[s];
    cur[s] = h->f16 ? lens[s] - 1 : 0;  // the rows path reads positions from its table; the chunk path moves cur_len itself
    h->plen[s] = lens[s];
  }
  IX_HIP(hipMemcpy(h->cur_len, cur, (size_t)n * 4, hipMemcpyHostToDevice));
  IX_HIP(hipMemcpy(h->gen_count, zero, (size_t)n * 4, hipMemcpyHostToDevice));
  IX_HIP(hipMemcpy(h->finished, zero, (size_t)n * 4, hipMemcpyHostToDevice));
  IX_HIP(hipMemcpy(h->n_kept, zero, (size_t)n * 4, hipMemcpyHostToDevice));
  if (h->f16) return q_prefill_rows(h, n, lens, st);
  // f32 (parity mode): slot after slot on the chunk path, into that slot's cache
  for (int s = 0; s < n; ++s) {
    IX_TRY(q_run(h, STEP_CHUNK, (lens[s] - 1) / PCH, st, s));
    IX_TRY(q_run(h, STEP_PRE, (lens[s] - 1) % PCH, st, s));
  }
  return IXTTS_OK;
}

static int q_check_slots(ixtts_qwen* h, int n, const char* who) {
  IX_ARG(n >= 1 && n <= h->n_slots, "%s: %d sequences on an engine of %d slots", who, n, h->n_slots);
  for (int s = 0; s < n; ++s) IX_ARG(h->plen[s] > 0 && h->kcs[s], "%s: slot %d has no prompt (call ixtts_qwen_prefill_slots)", who, s);
  return IXTTS_OK;
}

static int q_run_slots(ixtts_qwen* h, int n, int n_steps, hipStream_t st) {
  return n == 1 ? q_run(h, STEP_FULL, n_steps, st) : q_run(h, STEP_SLOTS, n_steps, st, n);
}

extern "C" int ixtts_qwen_step_slots(ixtts_qwen* h, int n, int n_steps, const ixtts_qwen_sampling* sc, void* stream) {
  Q_READY(h, "qwen_step_slots");
  IX_ARG(n_steps >= 0, "qwen_step_slots: n_steps %d", n_steps);
  IX_TRY(q_check_slots(h, n, "qwen_step_slots"));
  hipStream_t st = (hipStream_t)stream;
  IX_TRY(q_set_sampling(h, sc, st));
  return q_run_slots(h, n, n_steps, st);
}

extern "C" int ixtts_qwen_generate_slots(ixtts_qwen* h, int n, int max_new, const ixtts_qwen_sampling* sc, void* stream) {
  Q_READY(h, "qwen_generate_slots");
  IX_ARG(max_new >= 0, "qwen_generate_slots: max_new %d", max_new);
  IX_TRY(q_check_slots(h, n, "qwen_generate_slots"));
  hipStream_t st = (hipStream_t)stream;
  IX_TRY(q_set_sampling(h, sc, st));
  // a slot whose cache fills up stops by itself; the steps end with the slot that has the most room
  int room = 0;
  for (int s = 0; s < n; ++s) room = std::max(room, h->smax - h->plen[s]);
  max_new = std::min(max_new, room);
  int done = 0;
  while (done < max_new) {
    const int k = std::min(16, max_new - done);
    IX_TRY(q_run_slots(h, n, k, st));
    done += k;
    IX_HIP(hipStreamSynchronize(st));
    int f[MAXS] = {};
    IX_HIP(hipMemcpy(f, h->finished, (size_t)n * 4, hipMemcpyDeviceToHost));
    bool all = true;
    for (int s = 0; s < n; ++s) all = all && f[s] != 0;
    if (all) break;
  }
  IX_HIP(hipStreamSynchronize(st));
  return IXTTS_OK;
}

extern "C" int ixtts_qwen_draw(ixtts_qwen* h, uint64_t seed, int n, int32_t* ids, void* stream) {
  Q_READY(h, "qwen_draw");
  IX_ARG(ids && n >= 1 && n <= (1 << 24), "qwen_draw: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  int nk = 0;
  IX_HIP(hipStreamSynchronize(st));
  IX_HIP(hipMemcpy(&nk, h->n_kept, 4, hipMemcpyDeviceToHost));
  IX_ARG(nk >= 1, "qwen_draw: no decode step has selected a token yet");
  if (h->draws_cap < n) {
    if (h->draws) hipFree(h->draws);
    h->draws = nullptr, h->draws_cap = 0;
    IX_HIP(hipMalloc(&h->draws, (size_t)n * 4));
    h->draws_cap = n;
  }
  hipLaunchKernelGGL(qdraw_kernel, dim3((n + 255) / 256), dim3(256), 0, st, h->kept_id, h->kept_p, h->n_kept, (unsigned long long)seed, n, h->draws);
  IX_HIP(hipGetLastError());
  IX_HIP(hipStreamSynchronize(st));
  IX_HIP(hipMemcpy(ids, h->draws, (size_t)n * 4, hipMemcpyDeviceToHost));
  return IXTTS_OK;
}

extern "C" double ixtts_qwen_step_bytes(const ixtts_qwen* h, int S) {
  if (!h) return 0.0;
  const double D = h->D, qd = h->H * HDIM, kvd = h->KVH * HDIM, I = h->I;
  const double layer = ((qd + 2 * kvd) * D + D * qd + 3 * I * D) * h->esz;
  return h->L * layer + (double)h->V * D * h->esz + (double)h->L * 2.0 * kvd * S * 4.0;
}

extern "C" int ixtts_qwen_destroy(ixtts_qwen* h) {
  if (!h) return IXTTS_OK;
  hipDeviceSynchronize();
  q_free(h);
  delete h;
  return IXTTS_OK;
}
