// The online CLS pooling kernel (lt_model.h has its description), as text that lt_model.h includes once per geometry: no include
// guard.  The including file defines
//   LT_POOL_KERNEL       the kernel's name
//   LT_POOL_MAP_PARAMS   the parameters that say where the images' channel-last descriptor maps are
//   LT_POOL_MAP(image)   statements that define `const PoolElem* nhwc_img` and `Hc`, `Wc` of the sub-line's image from them, and
//                        PoolElem itself: the map's element type (float, f16_t or bf16_t)
//   LT_POOL_TPARAMS      further template parameters behind SPLIT (empty for the float32 kernels; `, class E` for the half ones)
// The uniform instantiation expands to the very text the kernel had before the ragged one existed, so it compiles to the same code
// (the shared-body-through-an-inlined-function form moved its FMA contraction and with it the last bits of the pooled rows).
template <int SPLIT LT_POOL_TPARAMS>
__global__ __launch_bounds__(256, 3) void LT_POOL_KERNEL(   // 3 = waves per SIMD the register allocation must allow
    const LinetrLineRec* __restrict__ recs, const int* __restrict__ sub2line_g, const float* __restrict__ cpnt,
    const float* __restrict__ a4, int64_t first_pad, int N, int T, LT_POOL_MAP_PARAMS,
    int align_corners, ClsPoolConst cc, float* __restrict__ pooled /*[N][4][544]*/, int reverse) {
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  // reverse: the LAST sub-lines first -- their a4 rows are the ones the token MLP wrote most recently and are still in the
  // Infinity Cache (a4 of a cfg3 batch is 298 MB, the cache 256 MB: walking forward finds none of it)
  const int n_fwd = SPLIT == 1 ? blockIdx.x * 4 + wv : blockIdx.x;
  if (n_fwd >= N) return;
  const int n = reverse ? N - 1 - n_fwd : n_fwd;
  const LinetrLineRec r = recs[sub2line_g[n]];
  const int j = n - r.first_sub;
  const int n_valid = min(T, r.n_tok - j * T);
  const int n_pad = T - n_valid;
  const int ntk = n_valid + (n_pad > 0 ? 1 : 0);
  const int64_t tok0 = (int64_t)r.first_tok + (int64_t)j * T;
  const int64_t padrow = first_pad + r.image;
  LT_POOL_MAP(r.image)
  f32x4 u[4], u2[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    u[h] = *reinterpret_cast<const f32x4*>(cc.U + h * D + lane * 4);
    u2[h] = *reinterpret_cast<const f32x4*>(cc.U2 + h * D + lane * 4);
  }
  // running state per head: max m, sum l, weight of the CLS key w0, pooled sums (this lane's 4 channels)
  float m[4], l[4], w0[4];
  f32x4 db[4], ab[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    m[h] = cc.s_cls[h] * LOG2E; l[h] = 1.f; w0[h] = 1.f;
    if (SPLIT > 1 && wv != 0) { m[h] = -INFINITY; l[h] = 0.f; w0[h] = 0.f; }   // the CLS key belongs to wave 0's share
    db[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    ab[h] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto row_of = [&](int jj) -> int64_t { return jj < n_valid ? tok0 + jj : padrow; };
  // The tap geometry of a token is wave-uniform and costs ~150 VALU instructions (two divisions, floor, clamps):
  // lane i computes it once for token chunk + i, and the loop below fetches a token's 4 offsets + 4 weights with
  // 8 v_readlane instead of recomputing them in all 64 lanes.
  int t_off[4];
  float t_w[4];
  auto fill_taps = [&](int chunk) {
    const int jj = chunk + lane;
    const int64_t row = row_of(jj < ntk ? jj : ntk - 1);
    tap_coords(cpnt[row * 2], cpnt[row * 2 + 1], Hc, Wc, align_corners, t_off, t_w);
  };
  auto issue = [&](int jj, TapSetT<PoolElem>& t, f32x4& a) {
    int off[4];
    float wt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      off[k] = __builtin_amdgcn_readlane(t_off[k], jj & 63);
      wt[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t_w[k]), jj & 63));
    }
    taps_load(nhwc_img, off, wt, lane, t);
    a = *reinterpret_cast<const f32x4*>(a4 + row_of(jj) * D + lane * 4);
  };
  TapSetT<PoolElem> cur, nxt;
  f32x4 a_cur, a_nxt;
  const int jj0 = SPLIT == 1 ? 0 : wv;
  fill_taps(0);
  if (jj0 < ntk) issue(jj0, cur, a_cur);
  for (int jj = jj0; jj < ntk; jj += SPLIT) {
    if (jj + SPLIT < ntk) {  // wave-uniform
      if (((jj + SPLIT) >> 6) != (jj >> 6)) fill_taps((jj + SPLIT) & ~63);
      issue(jj + SPLIT, nxt, a_nxt);
    }
    const f32x4 dv = taps_finish<true>(cur);
    const float mult = jj < n_valid ? 1.f : (float)n_pad;
    float sc[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      float p = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) p += dv[c] * u[h][c] + a_cur[c] * u2[h][c];
      sc[h] = p;
    }
    wave_sum_n<4>(sc);                      // the four head scores reduce together
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      // running softmax in the log2 domain: one v_exp_f32 per exponential (m / l / w0 are only ever used as ratios)
      const float sh = (sc[h] + cc.c_tok[h]) * LOG2E;
      if (__any(sh > m[h])) {   // wave-uniform (sh and m are): the running maximum moves on few tokens only
        const float alpha = __builtin_amdgcn_exp2f(m[h] - sh);
        m[h] = sh;
        l[h] *= alpha;
        w0[h] *= alpha;
#pragma unroll
        for (int c = 0; c < 4; ++c) { db[h][c] *= alpha; ab[h][c] *= alpha; }
      }
      const float e = __builtin_amdgcn_exp2f(sh - m[h]) * mult;
      l[h] += e;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        db[h][c] += e * dv[c];
        ab[h][c] += e * a_cur[c];
      }
    }
    cur = nxt;
    a_cur = a_nxt;
  }
  float* out = pooled + (int64_t)n * 4 * POOLW;
  if constexpr (SPLIT > 1) {
    // merge the four waves' states: wave h finishes head h
    __shared__ float st_ml[4][4][4];                        // [wave][head][m, l, w0, -]
    __shared__ f32x4 st_v[4][4][2][64];                     // [wave][head][d / a][lane]
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      if (lane == 0) { st_ml[wv][h][0] = m[h]; st_ml[wv][h][1] = l[h]; st_ml[wv][h][2] = w0[h]; }
      st_v[wv][h][0][lane] = db[h];
      st_v[wv][h][1][lane] = ab[h];
    }
    __syncthreads();
    const int h = wv;
    float M = st_ml[0][h][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, st_ml[w][h][0]);
    float L = 0.f, W0 = 0.f;
    f32x4 d = {0.f, 0.f, 0.f, 0.f}, a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float sc = __builtin_amdgcn_exp2f(st_ml[w][h][0] - M);     // a wave without tokens has m = -inf: weight 0
      L += st_ml[w][h][1] * sc;
      W0 += st_ml[w][h][2] * sc;
      const f32x4 dv = st_v[w][h][0][lane], av = st_v[w][h][1][lane];
#pragma unroll
      for (int c = 0; c < 4; ++c) { d[c] += dv[c] * sc; a[c] += av[c] * sc; }
    }
    const float inv = 1.f / L;
#pragma unroll
    for (int c = 0; c < 4; ++c) { d[c] *= inv; a[c] *= inv; }
    *reinterpret_cast<f32x4*>(out + h * POOLW + lane * 4) = d;
    *reinterpret_cast<f32x4*>(out + h * POOLW + 256 + lane * 4) = a;
    if (lane < 8) {  // [p_h0, 0 x 31]
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      if (lane == 0) z[0] = W0 * inv;
      *reinterpret_cast<f32x4*>(out + h * POOLW + 512 + lane * 4) = z;
    }
    return;
  }
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const float inv = 1.f / l[h];
    f32x4 d = db[h], a = ab[h];
#pragma unroll
    for (int c = 0; c < 4; ++c) { d[c] *= inv; a[c] *= inv; }
    *reinterpret_cast<f32x4*>(out + h * POOLW + lane * 4) = d;
    *reinterpret_cast<f32x4*>(out + h * POOLW + 256 + lane * 4) = a;
    if (lane < 8) {  // [p_h0, 0 x 31]
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      if (lane == 0) z[0] = w0[h] * inv;
      *reinterpret_cast<f32x4*>(out + h * POOLW + 512 + lane * 4) = z;
    }
  }
}
