// Neighbour-line ("signature") attention of one image per softmax domain (models/line_transformer.py:132-154) as separate
// launches behind the q/k/v GEMM: sig_attn_kernel (exact fp32 MFMA), sig_attn_split_kernel<NW> (split-bf16 MFMA) and
// sig_attn_small_kernel (its latency form for a few images).  The fused projection + attention kernel is lt_attn_fused.h; the
// pieces the kernels share are lt_attn_parts.h; the choice between them is sig_attn_plan (linetr_net.hip).
#pragma once
#include "lt_attn_parts.h"

namespace lt {

// ---------------------------------------------------------------------------------------------
// Neighbour-line ("signature") multi-head attention, one image = one softmax domain
// (models/line_transformer.py:132-154), exact fp32 MFMA: sig_attn_tile<false> (lt_attn_parts.h) on one buffer.
//
// grid (image, head, q-tile of ATT_QT = 128), block 256.
// qkv [N,768] = [q | k | v], each head-major (c = h*64+d; the reference's interleaved c = d*4+h is
// undone by permuting weight rows at load time) and q pre-scaled by 1/8 (exact, power of two).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sig_attn_kernel(const float* __restrict__ qkv, const int* __restrict__ cu_sub,
                                                       float* __restrict__ out /*[N][256] head-major*/) {
  const int img = blockIdx.x, head = blockIdx.y;
  const int n0 = cu_sub[img], Ni = cu_sub[img + 1] - n0;
  const int q0 = blockIdx.z * ATT_QT;
  if (q0 >= Ni) return;
  sig_attn_tile<false>(qkv, 768, qkv + 256, 768, qkv + 512, 768, n0, Ni, q0, head, out, D, nullptr);
}

// ---------------------------------------------------------------------------------------------
// Same attention with the two contractions on split-bf16 MFMA (3 planes / 6 products = fp32-faithful, see
// lt_gemm_split.h): v_mfma_f32_32x32x16_bf16 is 16x the rate of the fp32 MFMA, so QK^T + PV cost 48 x 32 cycles
// per 32-row kv chunk instead of 64 x 64.
//   * Q fragments: split once into VGPRs (12 x bf16x8).
//   * K tile in LDS as planes [kv][3][64 d] (row stride 400 B = 4*25 dwords -> conflict-free ds_read_b128).
//   * V tile in LDS row-major as planes [kv][3][64 d] like K (row stride 576 B); the PV B-operand P^T[kv][q] comes
//     straight from the S^T accumulator registers (k-slot e of step t is register 8t+e, i.e.
//     kv = 16t + 4*(lane>>5) + e for e<4 and +8 for e>=4), and the matching A operand V^T[d][kv] -- two runs of four kv
//     for one d -- is fetched with gfx950's transposing LDS read (v_frags_tr), so staging V costs three 8-byte stores per
//     thread instead of twelve 2-byte scatter stores into a transposed image.
//   * softmax stays fp32 and in-lane as in sig_attn_kernel.
// ---------------------------------------------------------------------------------------------
constexpr int ATS_RK = 3 * 128 + 16;   // K plane row stride (bytes)
constexpr int ATS_RV = 576;            // V plane row stride (bytes): 144 dwords = 16 (mod 64), see below

// The V^T fragments of the 16-wide kv step KV0 and the 32-wide d block DT by tr_reads (lt_attn_parts.h): V stays ROW-major in LDS
// ([kv][3 planes][64 d], staged with three 8-byte stores per thread like K).  `base` is the lane's byte address for kv0 = 0,
// plane 0, d block 0.  Bank check: a half-wave reads 4 rows x 64 bytes; with a row stride of 16 dwords (mod 64) the four rows
// land on four disjoint quarters of the 64 banks.
template <int KV0, int DT, bool WAIT = true>
__device__ __forceinline__ void v_frags_tr(unsigned base, u32x2 (&o)[3][2]) {
  tr_reads<KV0 * ATS_RV + DT * 64, (KV0 + 8) * ATS_RV + DT * 64, 128, WAIT>(base, o);
}

// NW waves per block = 32 NW query rows per block.  With 8 waves the K / V tiles of an (image, head) are split and
// staged once for up to 256 queries instead of once per 128.
// The 8-wave kernel is capped at 128 VGPRs so that TWO blocks share a CU (4 waves per SIMD) and fetches its K / V rows right
// before staging them -- the second block covers the latency -- instead of carrying a register prefetch.
// Measured at cfg3 (7 launches per step): 0.366 ms with one block per CU and the prefetch, 0.337 ms this way.
template <int NW>
__global__ __launch_bounds__(NW * 64, NW == 8 ? 4 : 1) void sig_attn_split_kernel(const float* __restrict__ qkv,
                                                                 const int* __restrict__ cu_sub,
                                                                 float* __restrict__ out /*[N][256] head-major*/) {
  __shared__ __attribute__((aligned(16))) unsigned char Ks[ATT_KT * ATS_RK];
  __shared__ __attribute__((aligned(16))) unsigned char Vs[ATT_KT * ATS_RV];
  const int img = blockIdx.x, head = blockIdx.y;
  const int n0 = cu_sub[img], Ni = cu_sub[img + 1] - n0;
  // the image's queries are dealt out EVENLY over the gridDim.z blocks of its (image, head), in whole waves: 599 queries on
  // three 256-query blocks are 7 + 7 + 5 busy waves instead of 8 + 8 + 3 (every block stages all K / V tiles either way)
  const int per = ((Ni + (int)gridDim.z - 1) / (int)gridDim.z + 31) / 32 * 32;     // <= NW * 32
  const int q0 = blockIdx.z * per;
  if (q0 >= Ni) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h2 = lane >> 5, lq = lane & 31;
  const int q = q0 + wave * 32 + lq;
  const bool wave_active = wave * 32 < per && q0 + wave * 32 < Ni;  // wave-uniform
  const float* base = qkv + (int64_t)n0 * 768;

  bf16x8 qf[4][3];
  {
    const int qr = q < Ni ? q : Ni - 1;
    const float* qp = base + (int64_t)qr * 768 + head * DH + h2 * 8;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      f32x4 x0 = *reinterpret_cast<const f32x4*>(qp + s * 16);
      f32x4 x1 = *reinterpret_cast<const f32x4*>(qp + s * 16 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { x0[e] *= LOG2E; x1[e] *= LOG2E; }   // scores in log2 units: exp -> v_exp_f32
      unsigned a[3], b[3], c[3], d[3];   // = q_frags / split8 (lt_attn_parts.h), written out: through them the 8-wave kernel's registers move
      split_pair<3>(x0[0], x0[1], a); split_pair<3>(x0[2], x0[3], b);
      split_pair<3>(x1[0], x1[1], c); split_pair<3>(x1[2], x1[3], d);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        union { bf16x8 v; unsigned w[4]; } u;
        u.w[0] = a[p]; u.w[1] = b[p]; u.w[2] = c[p]; u.w[3] = d[p];
        qf[s][p] = u.v;
      }
    }
  }
  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m = -INFINITY, l = 0.f;

  // lane address of the transposing V reads for kv0 = 0 (see v_frags_tr)
  const unsigned v_base = (unsigned)(size_t)(Vs + (((lane & 15) >> 2) + 4 * h2) * ATS_RV + (((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2);
  const int srow = tid >> 4, sc4 = (tid & 15) * 4;  // staging: 4 NW rows x 16 float4 per pass
  constexpr int NPASS = ATT_KT / (4 * NW);
  f32x4 kreg[NPASS], vreg[NPASS];
  auto fetch = [&](int t0) {
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      const int kv = t0 + srow + i * (4 * NW);
      kreg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      vreg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kv < Ni) {
        const float* p = base + (int64_t)kv * 768 + head * DH + sc4;
        kreg[i] = *reinterpret_cast<const f32x4*>(p + 256);
        vreg[i] = *reinterpret_cast<const f32x4*>(p + 512);
      }
    }
  };
  for (int t0 = 0; t0 < Ni; t0 += ATT_KT) {
    fetch(t0);                       // no register prefetch: the second resident block covers the latency instead
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      const int r = srow + i * (4 * NW);
      const f32x4 kx = kreg[i], vx = vreg[i];
      unsigned a[3], b[3];
      split_pair<3>(kx[0], kx[1], a);
      split_pair<3>(kx[2], kx[3], b);
#pragma unroll
      for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x2*>(Ks + r * ATS_RK + p * 128 + sc4 * 2) = u32x2{a[p], b[p]};
      split_pair<3>(vx[0], vx[1], a);
      split_pair<3>(vx[2], vx[3], b);
#pragma unroll
      for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x2*>(Vs + r * ATS_RV + p * 128 + sc4 * 2) = u32x2{a[p], b[p]};
    }
    __syncthreads();
    if (!wave_active) continue;
#pragma unroll
    for (int c = 0; c < ATT_KT / 32; ++c) {
      const int kv0 = t0 + c * 32;
      if (kv0 >= Ni) break;
      f32x16 st;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = 0.f;
      const unsigned char* kp = Ks + (c * 32 + lq) * ATS_RK + h2 * 16;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8 ka[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) ka[p] = *reinterpret_cast<const bf16x8*>(kp + p * 128 + s * 32);
        mma6(ka, qf[s], st);
      }
      if (kv0 + 32 > Ni) {   // wave-uniform: only the image's last chunk has keys past the end
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kv0 + (r & 3) + 8 * (r >> 2) + 4 * h2 >= Ni) st[r] = -INFINITY;
      }
      float mx = st[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
      mx = xor32_max(mx);
      const float m_new = fmaxf(m, mx);
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) { st[r] = __builtin_amdgcn_exp2f(st[r] - m_new); ps += st[r]; }
      ps = xor32_sum(ps);
      if (__any(m_new != m)) {      // wave-uniform: once the running max has settled the accumulators need no rescale
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);   // m = -inf on the first chunk -> 0
        l *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
      }
      l += ps;
      m = m_new;
      // P^T planes straight from the accumulator registers
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bf16x8 pp[3];
        {
          unsigned w[4][3];
#pragma unroll
          for (int e = 0; e < 4; ++e) split_pair<3>(st[8 * t + 2 * e], st[8 * t + 2 * e + 1], w[e]);
#pragma unroll
          for (int p = 0; p < 3; ++p) {
            union { bf16x8 v; unsigned u[4]; } x;
            x.u[0] = w[0][p]; x.u[1] = w[1][p]; x.u[2] = w[2][p]; x.u[3] = w[3][p];
            pp[p] = x.v;
          }
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          u32x2 vr[3][2];
          if (dt == 0) {
            if (c == 0) { if (t == 0) v_frags_tr<0, 0>(v_base, vr); else v_frags_tr<16, 0>(v_base, vr); }
            else        { if (t == 0) v_frags_tr<32, 0>(v_base, vr); else v_frags_tr<48, 0>(v_base, vr); }
          } else {
            if (c == 0) { if (t == 0) v_frags_tr<0, 1>(v_base, vr); else v_frags_tr<16, 1>(v_base, vr); }
            else        { if (t == 0) v_frags_tr<32, 1>(v_base, vr); else v_frags_tr<48, 1>(v_base, vr); }
          }
          bf16x8 va[3];
#pragma unroll
          for (int p = 0; p < 3; ++p) {
            union { bf16x8 v; unsigned u[4]; } x;
            x.u[0] = vr[p][0][0]; x.u[1] = vr[p][0][1]; x.u[2] = vr[p][1][0]; x.u[3] = vr[p][1][1];
            va[p] = x.v;
          }
          mma6(va, pp, dt == 0 ? o0 : o1);
        }
      }
    }
  }
  if (wave_active) {
    // O^T: a lane owns ONE query and 4-runs of d (d = 8 (r >> 2) + 4 h2 + (r & 3)).  One v_permlane32_swap per register
    // pair hands each half-wave the other half's 4-run, so a lane ends up with 8 consecutive d and stores them as two
    // dwordx4 (r02 stored 32 single dwords per lane: 32 rows x 4 B per instruction, a store-issue-bound tail).
    const float inv = 1.f / l;
    float* op = out + (int64_t)(n0 + (q < Ni ? q : Ni - 1)) * D + head * DH + 8 * h2;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = (dt == 0 ? o0[r] : o1[r]) * inv;
#pragma unroll
      for (int c = 0; c < 4; ++c) {        // (v[c], v[4 + c]) and (v[8 + c], v[12 + c]): upper half of the first <-> lower half of the second
        float a0 = v[c], b0 = v[4 + c], a1 = v[8 + c], b1 = v[12 + c];
        halves_swap(a0, b0);
        halves_swap(a1, b1);
        v[c] = a0; v[4 + c] = b0; v[8 + c] = a1; v[12 + c] = b1;
      }
      if (q < Ni) {
        // after the swaps v[0..7] = d 32 dt + 8 h2 .. + 8 and v[8..15] = d 32 dt + 16 + 8 h2 .. + 8
        *reinterpret_cast<f32x4*>(op + dt * 32) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(op + dt * 32 + 4) = f32x4{v[4], v[5], v[6], v[7]};
        *reinterpret_cast<f32x4*>(op + dt * 32 + 16) = f32x4{v[8], v[9], v[10], v[11]};
        *reinterpret_cast<f32x4*>(op + dt * 32 + 20) = f32x4{v[12], v[13], v[14], v[15]};
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Latency form of sig_attn_split_kernel for a few images (single pair): the KV range is split across the block's 4 waves
// as well.  grid (image, head, 32-query tile), 256 threads; wave w takes the 32-row KV chunks w, w+4, ... of its
// (image, head), stages them in a WAVE-PRIVATE LDS region (no block barrier in the loop), runs the same split-bf16
// QK^T / online softmax / PV as above, and the four partial (m, l, O) are merged through LDS at the end (exact: the
// softmax is rescaled to the common maximum).  A single 2 x 199-line pair launches 56 blocks of 4 waves whose critical
// path is 2 chunks, instead of 8 (or 32) blocks walking 7 chunks each.
// ---------------------------------------------------------------------------------------------
constexpr int ATL_RK = 3 * 128 + 16;   // K plane row stride (bytes): [kv][3][64 d]
constexpr int ATL_RV = 3 * 64 + 8;     // V^T plane row stride (bytes): [d][3][32 kv]
constexpr int ATL_WAVE_BYTES = 32 * ATL_RK + DH * ATL_RV;   // 12 800 + 12 800

__global__ __launch_bounds__(256) void sig_attn_small_kernel(const float* __restrict__ qkv, const int* __restrict__ cu_sub,
                                                             float* __restrict__ out /*[N][256] head-major*/,
                                                             int ldq /*row stride of qkv in floats: 768, or 1024 when q/k/v sit behind x_out*/) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * ATL_WAVE_BYTES];
  const int img = blockIdx.x, head = blockIdx.y;
  const int n0 = cu_sub[img], Ni = cu_sub[img + 1] - n0;
  const int q0 = blockIdx.z * 32;
  if (q0 >= Ni) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h2 = lane >> 5, lq = lane & 31;
  const int q = q0 + lq;
  const float* base = qkv + (int64_t)n0 * ldq;
  unsigned char* Ks = lds + wave * ATL_WAVE_BYTES;
  unsigned char* Vt = Ks + 32 * ATL_RK;

  bf16x8 qf[4][3];
  {
    const int qr = q < Ni ? q : Ni - 1;
    const float* qp = base + (int64_t)qr * ldq + head * DH + h2 * 8;
    q_frags(qp, qf);
  }
  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m = -INFINITY, l = 0.f;

  // staging of one 32-row chunk by one wave: 16 lanes x float4 per row, 4 rows per pass, 8 passes
  const int srow = lane >> 4, sc4 = (lane & 15) * 4;
  f32x4 kreg[8], vreg[8];
  auto fetch = [&](int kv0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kv = kv0 + srow + 4 * i;
      kreg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      vreg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kv < Ni) {
        const float* p = base + (int64_t)kv * ldq + head * DH + sc4;
        kreg[i] = *reinterpret_cast<const f32x4*>(p + 256);
        vreg[i] = *reinterpret_cast<const f32x4*>(p + 512);
      }
    }
  };
  if (wave * 32 < Ni) fetch(wave * 32);
  for (int kv0 = wave * 32; kv0 < Ni; kv0 += 128) {       // wave-uniform trip count
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = srow + 4 * i;
      unsigned a[3], b[3];
      split_pair<3>(kreg[i][0], kreg[i][1], a);
      split_pair<3>(kreg[i][2], kreg[i][3], b);
#pragma unroll
      for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x2*>(Ks + r * ATL_RK + p * 128 + sc4 * 2) = u32x2{a[p], b[p]};
      split_pair<3>(vreg[i][0], vreg[i][1], a);
      split_pair<3>(vreg[i][2], vreg[i][3], b);
#pragma unroll
      for (int p = 0; p < 3; ++p) {  // transposed: element (kv=r, d=sc4+j) -> Vt[d][p][r]
        unsigned short* col = reinterpret_cast<unsigned short*>(Vt + p * 64 + r * 2);
        col[(sc4 + 0) * (ATL_RV / 2)] = (unsigned short)(a[p] & 0xffffu);
        col[(sc4 + 1) * (ATL_RV / 2)] = (unsigned short)(a[p] >> 16);
        col[(sc4 + 2) * (ATL_RV / 2)] = (unsigned short)(b[p] & 0xffffu);
        col[(sc4 + 3) * (ATL_RV / 2)] = (unsigned short)(b[p] >> 16);
      }
    }
    if (kv0 + 128 < Ni) fetch(kv0 + 128);
    __builtin_amdgcn_wave_barrier();     // compiler-only: wave-private LDS, executed in order
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
    const unsigned char* kp = Ks + lq * ATL_RK + h2 * 16;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8 ka[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) ka[p] = *reinterpret_cast<const bf16x8*>(kp + p * 128 + s * 32);
      mma6(ka, qf[s], st);
    }
    if (kv0 + 32 > Ni) {          // (written out in every kernel: through a shared helper their instructions move)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kv0 + (r & 3) + 8 * (r >> 2) + 4 * h2 >= Ni) st[r] = -INFINITY;
    }
    float mx = st[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
    mx = xor32_max(mx);
    const float m_new = fmaxf(m, mx);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { st[r] = __builtin_amdgcn_exp2f(st[r] - m_new); ps += st[r]; }
    ps = xor32_sum(ps);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);   // m = -inf on the first chunk -> 0; unconditional (one chunk or two per wave)
    l = l * alpha + ps;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
    m = m_new;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      bf16x8 pp[3];
      split_p(st, t, pp);
      const unsigned char* vp = Vt + lq * ATL_RV + (16 * t + 4 * h2) * 2;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        bf16x8 va[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const u32x2 lo = *reinterpret_cast<const u32x2*>(vp + dt * 32 * ATL_RV + p * 64);
          const u32x2 hi = *reinterpret_cast<const u32x2*>(vp + dt * 32 * ATL_RV + p * 64 + 16);
          union { bf16x8 v; unsigned u[4]; } x;
          x.u[0] = lo[0]; x.u[1] = lo[1]; x.u[2] = hi[0]; x.u[3] = hi[1];
          va[p] = x.v;
        }
        mma6(va, pp, dt == 0 ? o0 : o1);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  // ---- merge the four partial results: O = sum_w 2^(m_w - M) O_w / sum_w 2^(m_w - M) l_w
  __syncthreads();                                   // all staging regions are dead
  float* Op = reinterpret_cast<float*>(lds);         // [4][64 d][33]  (q padded to 33)
  float* ML = Op + 4 * 64 * 33;                      // [4][2][32]
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int d = (r & 3) + 8 * (r >> 2) + 4 * h2;
    Op[(wave * 64 + d) * 33 + lq] = o0[r];
    Op[(wave * 64 + d + 32) * 33 + lq] = o1[r];
  }
  if (h2 == 0) { ML[(wave * 2 + 0) * 32 + lq] = m; ML[(wave * 2 + 1) * 32 + lq] = l; }
  __syncthreads();
  const int oq = tid >> 3, od = (tid & 7) * 8;       // thread -> (query, 8 consecutive d)
  if (q0 + oq < Ni) {
    float mw[4], M = -INFINITY, L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) { mw[w] = ML[(w * 2) * 32 + oq]; M = fmaxf(M, mw[w]); }
    float sc[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      sc[w] = mw[w] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw[w] - M);   // a wave without any chunk contributes nothing
      L += sc[w] * ML[(w * 2 + 1) * 32 + oq];
    }
    const float inv = 1.f / L;
    float res[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) a += sc[w] * Op[(w * 64 + od + e) * 33 + oq];
      res[e] = a * inv;
    }
    float* op = out + (int64_t)(n0 + q0 + oq) * D + head * DH + od;
    *reinterpret_cast<f32x4*>(op) = f32x4{res[0], res[1], res[2], res[3]};
    *reinterpret_cast<f32x4*>(op + 4) = f32x4{res[4], res[5], res[6], res[7]};
  }
}

}  // namespace lt
