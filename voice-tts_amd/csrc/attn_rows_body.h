// attn_rows_body.h -- NO include guard: the statements of the row-at-a-time causal attention of gpt_rows.hip, included into the body of
// attn_rows_kernel, attn_rows_packed_kernel and attn_rows_packed_rebased_kernel.  In scope at the include: KVT, OT, AttnRowsArgs a, and
// the macros ROWS_ROW = the query row within the sequence and ROWS_K0 = the key offset: the sweep sees cache position ROWS_K0 + k as
// its position k (pointers advanced by ROWS_K0 rows, bounds and clamp shortened by as much).  Kept as text and not as a __device__
// function: behind a function parameter the compiler allocates the one-sequence kernel differently.
  constexpr int NW = 4;
  using LY = KVLayout<KVT>;
  __shared__ float sm[NW][LY::LPP][2 + LY::DPL];
  const int hh = blockIdx.x, row = ROWS_ROW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dp = lane % LY::LPP;
  float qv[LY::DPL];
  load_q_slice<KVT>(a.q + (size_t)row * a.D + hh * HD, dp, qv);
  const KVT* kb = reinterpret_cast<const KVT*>(a.kcache) + ((size_t)hh * a.smax + ROWS_K0) * HD + dp * LY::DPL;
  const KVT* vb = reinterpret_cast<const KVT*>(a.vcache) + ((size_t)hh * a.smax + ROWS_K0) * HD + dp * LY::DPL;
  SoftAcc<LY::DPL> st;
  st.init();
  const int lo0 = a.valid_from - ROWS_K0, hi0 = a.pos0 - ROWS_K0 + row + 1;
  attn_sweep<KVT, NW, 8>(st, kb, vb, qv, a.smax - ROWS_K0, wave, lane, [&](int& lo, int& hi) {
    lo = lo0;
    hi = hi0;
  });
  const float o = attn_merge<KVT, NW>(st, sm, wave, lane);
  if (threadIdx.x < 64) store_kv(reinterpret_cast<OT*>(a.out) + (size_t)row * a.D + hh * HD + threadIdx.x, o);
