// attn_decode_device.h -- body of the single-query decode attention (rotary + KV append + attention),
// shared by attention.hip (stand-alone launch) and gemm.hip (decode_attn_gemv_kernel: co-launched with a GEMV).
#pragma once
#include "common.h"
#include "gemm_device.h"

// ---------------------------------------------------------------------------
// decode attention: one query per (b,h); ctx = pos + 1 keys, pos = d_pos[b * pos_stride]
// (pos_stride 0: one position for the batch; 1: one per row -- right-padded prompts of
// different lengths).  grid B*H, 256 thr.
//   FUSED = false: q [B,H,256] already rotated, K/V already appended.
//   FUSED = true : reads the fused qkv row [B, 3*H*256] of the new token, applies
//                  the rotary to q and k at angle row pos, appends k,v to the cache
//                  at pos and attends over [0, pos] -- one launch instead of two.
// Scores: S^T[key][.] = K . q^T on the MFMA (16 keys per wave step, all 8 K
// fragment loads of a step in flight at once, no cross-lane reductions); the 16
// "query columns" of the B operand all carry the same q.  PV: VALU, lane = 4
// dims, 8 keys in flight per wave step (V rows are coalesced 512-B reads).
// ---------------------------------------------------------------------------
constexpr int DEC_MAX_CTX = 4096;

constexpr int ATTN_DEC_LDS = DEC_MAX_CTX * 4 + 4 * 256 * 4 + 8 * 4 + 256 * 2 + 32;

struct AttnDecodeParams {
  const mg_bf16* qin; mg_bf16* kcache; mg_bf16* vcache; mg_bf16* out;
  int H, Smax; const int* d_pos; int rot_dim; const float* sin_t; const float* cos_t;
  int64_t ld_out = 0;      // row stride of `out` in elements (0 = H * 256)
  int pos_stride = 0;      // position of row b = d_pos[b * pos_stride]
};

// Shared session prefix (attn_decode_body<.., SHARED = true> only; a kernel argument of its own, so that the kernels of the
// existing entry points keep their argument block): the cache holds the rows' OWN positions, absolute position p >= n_prefix at
// own index p - n_prefix; `part` holds the prefix partials of attn_prefix_body, n_chunk per (b, h).
struct AttnSharedParams {
  int n_prefix = 0, n_chunk = 0;
  const float* part = nullptr;
};

// The rotary of 8 dims [d0, d0 + 8) of a q or k row at angle row `pos` (GPT-J: neighbouring pairs), in fp32, rounded to bf16 once.
// One statement of it for the decode body and the prefix-partials kernel, so that both rotate q to the same bits.
MG_DEV u32x4 rotary8_at(u32x4 v, const float* __restrict__ sin_t, const float* __restrict__ cos_t, int pos, int rot_dim, int d0) {
  const int half_rot = rot_dim >> 1;
  const float* sp = sin_t + (int64_t)pos * half_rot + (d0 >> 1);
  const float* cp = cos_t + (int64_t)pos * half_rot + (d0 >> 1);
#pragma unroll
  for (int pi = 0; pi < 4; ++pi) {
    const float sn = sp[pi], cs = cp[pi], x0 = bflo(v[pi]), x1 = bfhi(v[pi]);
    v[pi] = pack2bf(x0 * cs - x1 * sn, x1 * cs + x0 * sn);
  }
  return v;
}

// ---------------------------------------------------------------------------
// Shared session prefix, kernel 1 (DESIGN.md "Shared session prefix"): the partial attention of ALL B <= 16 batch rows over one
// chunk of PREFIX_CHUNK keys of the one prefix [H, n_prefix, 256] that every row has in front of its own positions.
// Workgroup (h, c), 256 threads.  Row b's rotated q is B-operand column b of the score MFMA (columns >= B are zero), so one set
// of K fragment loads scores the chunk for every row; wave w takes keys [16 w, 16 w + 16) of the chunk.  Per row over the chunk:
// m = max score, l = sum exp(s - m), o = sum exp(s - m) v in fp32, unnormalised -- PV on the VALU with fp32 weights (lane = 4 dims x
// 16 rows of accumulators, every V element loaded once), the four waves' sums added in one fixed order.  Keys >= n_prefix of the last
// chunk are masked (weight 0; their loads are clamped to key n_prefix - 1 and never enter a sum).  Written with plain vector stores:
// part[((b H + h) n_chunk + c) PREFIX_PART + {0..255: o, 256: m, 257: l}].  The split depends on n_prefix alone.
// ---------------------------------------------------------------------------
constexpr int PREFIX_CHUNK = 64;
constexpr int PREFIX_PART = 264;                 // floats per (b, h, chunk): 256 o, m, l, 6 unused (16-byte rows)
constexpr int PREFIX_QLD = 256 + 8;              // LDS row stride of q in bf16 (528 B: the 16 rows start in different banks)
constexpr int ATTN_PREFIX_LDS = 16 * PREFIX_QLD * 2 + PREFIX_CHUNK * 16 * 4 + 2 * 16 * 256 * 4;

struct AttnPrefixParams {
  const mg_bf16* qkv; const mg_bf16* kpre; const mg_bf16* vpre; float* part;
  int B, H, n_prefix, n_chunk, Spre; const int* d_pos; int rot_dim; const float* sin_t; const float* cos_t; int pos_stride;
};

MG_DEV void attn_prefix_body(const AttnPrefixParams& P, int h, int c, char* lds) {
  constexpr int DH = 256;
  mg_bf16* qs = (mg_bf16*)lds;                                              // [16][PREFIX_QLD]
  float* pT = (float*)(lds + 16 * PREFIX_QLD * 2);                          // [PREFIX_CHUNK][16]: score, then weight, of (key, row)
  float* red = pT + PREFIX_CHUNK * 16;                                      // [2][16 rows][256]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int B = P.B, H = P.H, n_prefix = P.n_prefix;
  const int dmodel = H * DH;
  // ---- q of every row, rotated at the row's own position, into LDS; rows >= B are zero and nothing of them is read ----
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int b = it * 8 + (tid >> 5), d0 = (tid & 31) * 8;
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (b < B) {
      v = *(const u32x4*)(P.qkv + (int64_t)b * 3 * dmodel + h * DH + d0);
      if (d0 < P.rot_dim) v = rotary8_at(v, P.sin_t, P.cos_t, max(P.d_pos[b * P.pos_stride], n_prefix), P.rot_dim, d0);
    }
    *(u32x4*)(qs + b * PREFIX_QLD + d0) = v;
  }
  __syncthreads();
  // ---- scores of the wave's 16 keys against the 16 rows: lane (li, lq) ends with row li, keys lq * 4 + r ----
  const mg_bf16* kb = P.kpre + (int64_t)h * P.Spre * DH;
  const mg_bf16* vb = P.vpre + (int64_t)h * P.Spre * DH;
  const int k0 = c * PREFIX_CHUNK + wave * 16;                              // the wave's first key
  {
    const mg_bf16* kp = kb + (int64_t)min(k0 + li, n_prefix - 1) * DH + lq * 8;
    bf16x8 kf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) kf[ks] = *(const bf16x8*)(kp + ks * 32);
    f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
      s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks], *(const bf16x8*)(qs + li * PREFIX_QLD + ks * 32 + lq * 8), s, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = wave * 16 + lq * 4 + r;
      pT[t * 16 + li] = c * PREFIX_CHUNK + t < n_prefix ? s[r] * 0.0625f : -1e30f;
    }
  }
  __syncthreads();
  // ---- per row: maximum and weights over the chunk; 16 threads per row, 4 keys each ----
  {
    const int b = tid >> 4, j = tid & 15;
    float sv[4], mx = -1e30f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { sv[r] = pT[(j * 4 + r) * 16 + b]; mx = fmaxf(mx, sv[r]); }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sm = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = c * PREFIX_CHUNK + j * 4 + r < n_prefix ? __expf(sv[r] - mx) : 0.f;
      pT[(j * 4 + r) * 16 + b] = e;
      sm += e;
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) sm += __shfl_xor(sm, o);
    if (j == 0 && b < B) {
      float* pp = P.part + (((int64_t)b * H + h) * P.n_chunk + c) * PREFIX_PART + DH;
      pp[0] = mx; pp[1] = sm;
    }
  }
  __syncthreads();
  // ---- PV: the wave's 16 keys, lane = dims [4 lane, 4 lane + 4) x 16 rows; all 16 V loads in flight at once ----
  float acc[16][4];
#pragma unroll
  for (int b = 0; b < 16; ++b) { acc[b][0] = acc[b][1] = acc[b][2] = acc[b][3] = 0.f; }
  u32x2 w[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) w[u] = *(const u32x2*)(vb + (int64_t)min(k0 + u, n_prefix - 1) * DH + lane * 4);
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const float v0 = bflo(w[u][0]), v1 = bfhi(w[u][0]), v2 = bflo(w[u][1]), v3 = bfhi(w[u][1]);
    const float* pr = pT + (wave * 16 + u) * 16;                            // weight 0 for a masked key
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (g * 4 < B) {
        const f32x4 p4 = *(const f32x4*)(pr + g * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[g * 4 + r][0] += p4[r] * v0; acc[g * 4 + r][1] += p4[r] * v1;
          acc[g * 4 + r][2] += p4[r] * v2; acc[g * 4 + r][3] += p4[r] * v3;
        }
      }
    }
  }
  // the four waves' sums, (w0 + w2) + (w1 + w3), through 32 KB of LDS; wave 0 ends with every row's o and stores rows < B
  auto put = [&](int slot) {
#pragma unroll
    for (int b = 0; b < 16; ++b) *(f32x4*)(red + (slot * 16 + b) * DH + lane * 4) = (f32x4){acc[b][0], acc[b][1], acc[b][2], acc[b][3]};
  };
  auto add = [&](int slot) {
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const f32x4 o = *(const f32x4*)(red + (slot * 16 + b) * DH + lane * 4);
      acc[b][0] += o[0]; acc[b][1] += o[1]; acc[b][2] += o[2]; acc[b][3] += o[3];
    }
  };
  if (wave >= 2) put(wave - 2);
  __syncthreads();
  if (wave < 2) add(wave);
  __syncthreads();
  if (wave == 1) put(0);
  __syncthreads();
  if (wave == 0) {
    add(0);
#pragma unroll
    for (int b = 0; b < 16; ++b)
      if (b < B)
        *(f32x4*)(P.part + (((int64_t)b * H + h) * P.n_chunk + c) * PREFIX_PART + lane * 4) = (f32x4){acc[b][0], acc[b][1], acc[b][2], acc[b][3]};
  }
}

// Device body: `bh` = (batch, head) index, `lds` = ATTN_DEC_LDS bytes of scratch (16-byte aligned).
// SHARED (FUSED only; shared session prefix, kernel 2; its fields are `S`): the cache holds the row's own positions -- k, v are
// appended at own index pos - n_prefix (a pos < n_prefix counts as n_prefix; a pos >= n_prefix + Smax skips the row like a position
// outside [0, Smax) in the plain mode: include/magma_hip.h "Device-resident indices"), the row attends over its own keys exactly as above,
// and the unnormalised result (maximum m, sum l, o) is merged with the row's n_chunk prefix partials in ascending chunk order
// under one maximum M: out = (e^(m - M) o + sum_c e^(m_c - M) o_c) / (e^(m - M) l + sum_c e^(m_c - M) l_c), rounded to bf16 once.
template <bool FUSED, bool SHARED = false>
MG_DEV void attn_decode_body(const AttnDecodeParams& P, int bh, char* lds, const AttnSharedParams& S = AttnSharedParams{}) {
  constexpr int DH = 256;
  const mg_bf16* __restrict__ qin = P.qin;
  mg_bf16* __restrict__ kcache = P.kcache;
  mg_bf16* __restrict__ vcache = P.vcache;
  mg_bf16* __restrict__ out = P.out;
  const int H = P.H, Smax = P.Smax, rot_dim = P.rot_dim;
  const int* __restrict__ d_pos = P.d_pos;
  const float* __restrict__ sin_t = P.sin_t;
  const float* __restrict__ cos_t = P.cos_t;
  mg_bf16* qs = (mg_bf16*)lds;                                   // 512 B (first: 16-byte aligned)
  float* sc = (float*)(lds + 512);
  float* red = sc + DEC_MAX_CTX;
  float* wred = red + 4 * DH;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int b = bh / H, h = bh - b * H;
  const int64_t out_off = P.ld_out ? (int64_t)b * P.ld_out + (int64_t)h * DH : (int64_t)bh * DH;
  static_assert(!SHARED || FUSED, "the shared-prefix mode is the fused body");
  const int pos = SHARED ? max(d_pos[b * P.pos_stride], S.n_prefix) : d_pos[b * P.pos_stride];    // the rotary angle
  const int own = SHARED ? pos - S.n_prefix : pos;                                                 // the cache index of the new token
  // d_pos is device-resident and no entry point can validate it: a row whose index lies outside [0, Smax) appends nothing, attends
  // over nothing and leaves its output row as it is.  One unsigned compare, uniform over the workgroup (one (b, h) each), in front
  // of the first barrier and of every address formed from `own` or `pos` (SHARED: pos >= n_prefix >= 1, the difference cannot wrap).
  if ((unsigned)own >= (unsigned)Smax) return;
  const int ctx = min(own + 1, min(Smax, DEC_MAX_CTX));
  mg_bf16* kb = kcache + (int64_t)bh * Smax * DH;
  mg_bf16* vb = vcache + (int64_t)bh * Smax * DH;
  if (FUSED) {
    // threads 0..31: q chunks, 32..63: k chunks, 64..95: v chunks (8 dims each)
    const int dmodel = H * DH;
    if (tid < 96) {
      const int which = tid >> 5, c = tid & 31, d0 = c * 8;
      u32x4 v = *(const u32x4*)(qin + (int64_t)b * 3 * dmodel + which * dmodel + h * DH + d0);
      if (which < 2 && d0 < rot_dim) v = rotary8_at(v, sin_t, cos_t, pos, rot_dim, d0);
      if (which == 0) *(u32x4*)(qs + d0) = v;
      else if (which == 1) *(u32x4*)(kb + (int64_t)own * DH + d0) = v;
      else *(u32x4*)(vb + (int64_t)own * DH + d0) = v;
    }
    __threadfence_block();
  } else {
    if (tid < 32) *(u32x4*)(qs + tid * 8) = *(const u32x4*)(qin + (int64_t)bh * DH + tid * 8);
  }
  __syncthreads();
  // ---- phase 1: scores on the MFMA, 16 keys per wave step ----
  bf16x8 qf[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) qf[ks] = *(const bf16x8*)(qs + ks * 32 + lq * 8);
  for (int t0 = wave * 16; t0 < ctx; t0 += 64) {
    const int key = min(t0 + li, ctx - 1);
    const mg_bf16* kp = kb + (int64_t)key * DH + lq * 8;
    bf16x8 kf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) kf[ks] = *(const bf16x8*)(kp + ks * 32);
    f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks], qf[ks], s, 0, 0, 0);
    if (li == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = t0 + lq * 4 + r;
        if (t < ctx) sc[t] = s[r] * 0.0625f;
      }
    }
  }
  __syncthreads();
  // ---- phase 2: softmax statistics ----
  float mx = -1e30f;
  for (int t = tid; t < ctx; t += 256) mx = fmaxf(mx, sc[t]);
  mx = wave_max(mx);
  if (lane == 0) wred[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
  float sm = 0.f;
  for (int t = tid; t < ctx; t += 256) {
    const float e = __expf(sc[t] - mx);
    sc[t] = e;
    sm += e;
  }
  sm = wave_sum(sm);
  if (lane == 0) wred[4 + wave] = sm;
  __syncthreads();
  const float inv = 1.0f / (wred[4] + wred[5] + wred[6] + wred[7]);
  // ---- phase 3: o = sum_t p[t] V[t]; wave w takes keys == w mod 4, 8 keys in flight ----
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int t0 = wave; t0 < ctx; t0 += 32) {
    u32x2 w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = min(t0 + u * 4, ctx - 1);
      w[u] = *(const u32x2*)(vb + (int64_t)t * DH + lane * 4);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = t0 + u * 4;
      const float pt = t < ctx ? sc[t] : 0.f;
      acc[0] += pt * bflo(w[u][0]); acc[1] += pt * bfhi(w[u][0]);
      acc[2] += pt * bflo(w[u][1]); acc[3] += pt * bfhi(w[u][1]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave * DH + lane * 4 + r] = acc[r];
  __syncthreads();
  if constexpr (SHARED) {
    // merge with the prefix partials: thread = one dim; m, l of a chunk are the same address for every thread
    const float* pp = S.part + (int64_t)bh * S.n_chunk * PREFIX_PART;
    float M = mx;
    for (int c = 0; c < S.n_chunk; ++c) M = fmaxf(M, pp[c * PREFIX_PART + DH]);
    const float w_own = __expf(mx - M);
    float num = w_own * (red[tid] + red[DH + tid] + red[2 * DH + tid] + red[3 * DH + tid]);
    float den = w_own * (wred[4] + wred[5] + wred[6] + wred[7]);
    for (int c = 0; c < S.n_chunk; ++c) {
      const float wc = __expf(pp[c * PREFIX_PART + DH] - M);      // underflows to an exact 0; o_c and l_c are finite
      num += wc * pp[c * PREFIX_PART + tid];
      den += wc * pp[c * PREFIX_PART + DH + 1];
    }
    out[out_off + tid] = f2bf(num / den);
    return;
  }
  const float v = (red[tid] + red[DH + tid] + red[2 * DH + tid] + red[3 * DH + tid]) * inv;
  out[out_off + tid] = f2bf(v);
}

// ---------------------------------------------------------------------------
// Chunk decode attention (DESIGN.md "Speculative decoding"): the fused body for NQ consecutive positions of one sequence, the NQ
// rows b * NQ + t of the fused qkv [B * NQ, 3*H*256].  Row t sits at position p = pos_b + t and is live iff (unsigned)p < Smax (the
// guard of the single-query body, per row: a dead row appends nothing, attends over nothing and leaves its out row as it is).
// All live rows' q and k are rotated at their own angle rows and k, v appended at their positions; after the barrier query t attends
// over keys [0, pos_b + t].  Query t is B-operand column t of the score MFMA, so one set of K fragment loads per 16 keys scores
// every query (lanes li < NQ keep their column); softmax and PV are the single-query body's, per query and in its order, every V
// load shared by the NQ queries -- a key beyond a query's own context enters its sum with weight exactly 0.f.  An element of the
// MFMA result depends on its own A row and B column alone, the statistics are reduced per query as there, and acc + 0.f * v = acc
// for a finite v: out and both caches have the bits of NQ successive single-query launches with row t fed at position pos_b + t.
// LDS (dynamic, sized by the launch's Smax): q [NQ][DEC_CHUNK_QLD] bf16, statistics [NQ][8], scores [NQ][Smax rounded up to 4]
// fp32, the four waves' PV sums [4][NQ][256] fp32 (last, so that the PV loop's look-ahead past a score row stays inside the block).
// ---------------------------------------------------------------------------
constexpr int DEC_CHUNK_MAX_Q = 8;
constexpr int DEC_CHUNK_QLD = 256 + 8;           // LDS row stride of q in bf16 (528 B: the rows start in different banks)
constexpr int DEC_CHUNK_MAX_LDS = 160 * 1024;    // LDS of one workgroup on gfx950

static inline int64_t attn_chunk_lds_bytes(int nq, int Smax) {
  return (int64_t)nq * (DEC_CHUNK_QLD * 2 + 8 * 4 + (int64_t)((Smax + 3) & ~3) * 4 + 4 * 256 * 4);
}

template <int NQ>
MG_DEV void attn_decode_chunk_body(const AttnDecodeParams& P, int bh, char* lds) {
  constexpr int DH = 256;
  static_assert(NQ >= 2 && NQ <= DEC_CHUNK_MAX_Q, "2 to 8 queries per sequence");
  const mg_bf16* __restrict__ qin = P.qin;
  mg_bf16* __restrict__ out = P.out;
  const int H = P.H, Smax = P.Smax, rot_dim = P.rot_dim;
  const int scld = (Smax + 3) & ~3;
  mg_bf16* qs = (mg_bf16*)lds;                                   // [NQ][DEC_CHUNK_QLD] (first: 16-byte aligned)
  float* wred = (float*)(lds + NQ * DEC_CHUNK_QLD * 2);          // [NQ][8]
  float* sc = wred + NQ * 8;                                     // [NQ][scld]
  float* red = sc + NQ * scld;                                   // [4][NQ][DH]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int b = bh / H, h = bh - b * H;
  const int64_t ld_out = P.ld_out ? P.ld_out : (int64_t)H * DH;
  const unsigned upos = (unsigned)P.d_pos[b * P.pos_stride];
  // The per-row guard: the sum is unsigned (no signed wrap in front of the compare), and nothing is formed from a position that
  // fails it.  ctx_of(t) = the keys query t attends over, 0 for a dead row; a live row's position is upos + t < Smax.
  auto ctx_of = [&](int t) -> int { const unsigned p = upos + (unsigned)t; return p < (unsigned)Smax ? (int)p + 1 : 0; };
  int ctx_max = 0;
#pragma unroll
  for (int t = 0; t < NQ; ++t) ctx_max = max(ctx_max, ctx_of(t));
  if (ctx_max == 0) return;                                      // uniform over the workgroup, in front of the first barrier
  mg_bf16* kb = P.kcache + (int64_t)bh * Smax * DH;
  mg_bf16* vb = P.vcache + (int64_t)bh * Smax * DH;
  {
    // item = (row t, which of q / k / v, 8 dims): 96 per row as in the single-query body
    const int dmodel = H * DH;
    for (int i = tid; i < NQ * 96; i += 256) {
      const int t = i / 96, r = i - t * 96, which = r >> 5, d0 = (r & 31) * 8;
      const int ctx = ctx_of(t);
      if (ctx == 0) {                                            // a dead row: its MFMA column is zero and nothing of it is read
        if (which == 0) *(u32x4*)(qs + t * DEC_CHUNK_QLD + d0) = (u32x4){0u, 0u, 0u, 0u};
        continue;
      }
      const int p = ctx - 1;
      u32x4 v = *(const u32x4*)(qin + (int64_t)(b * NQ + t) * 3 * dmodel + which * dmodel + h * DH + d0);
      if (which < 2 && d0 < rot_dim) v = rotary8_at(v, P.sin_t, P.cos_t, p, rot_dim, d0);
      if (which == 0) *(u32x4*)(qs + t * DEC_CHUNK_QLD + d0) = v;
      else if (which == 1) *(u32x4*)(kb + (int64_t)p * DH + d0) = v;
      else *(u32x4*)(vb + (int64_t)p * DH + d0) = v;
    }
    __threadfence_block();
  }
  __syncthreads();
  // ---- phase 1: scores on the MFMA, 16 keys per wave step; column li = query li ----
  const int my_ctx = li < NQ ? ctx_of(li) : 0;
  bf16x8 qf[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) qf[ks] = *(const bf16x8*)(qs + min(li, NQ - 1) * DEC_CHUNK_QLD + ks * 32 + lq * 8);
  for (int t0 = wave * 16; t0 < ctx_max; t0 += 64) {
    const int key = min(t0 + li, ctx_max - 1);
    const mg_bf16* kp = kb + (int64_t)key * DH + lq * 8;
    bf16x8 kf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) kf[ks] = *(const bf16x8*)(kp + ks * 32);
    f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks], qf[ks], s, 0, 0, 0);
    if (li < NQ) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = t0 + lq * 4 + r;
        if (t < my_ctx) sc[li * scld + t] = s[r] * 0.0625f;
      }
    }
  }
  __syncthreads();
  // ---- phase 2: softmax statistics, per query ----
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int ctx = ctx_of(q);
    float mx = -1e30f;
    for (int t = tid; t < ctx; t += 256) mx = fmaxf(mx, sc[q * scld + t]);
    mx = wave_max(mx);
    if (lane == 0) wred[q * 8 + wave] = mx;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int ctx = ctx_of(q);
    const float mx = fmaxf(fmaxf(wred[q * 8 + 0], wred[q * 8 + 1]), fmaxf(wred[q * 8 + 2], wred[q * 8 + 3]));
    float sm = 0.f;
    for (int t = tid; t < ctx; t += 256) {
      const float e = __expf(sc[q * scld + t] - mx);
      sc[q * scld + t] = e;
      sm += e;
    }
    sm = wave_sum(sm);
    if (lane == 0) wred[q * 8 + 4 + wave] = sm;
  }
  __syncthreads();
  // ---- phase 3: o_q = sum_t p_q[t] V[t]; wave w takes keys == w mod 4, 8 keys in flight, every V load used by all NQ queries ----
  float acc[NQ][4];
  int ctxs[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) { acc[q][0] = acc[q][1] = acc[q][2] = acc[q][3] = 0.f; ctxs[q] = ctx_of(q); }
  for (int t0 = wave; t0 < ctx_max; t0 += 32) {
    u32x2 w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = min(t0 + u * 4, ctx_max - 1);
      w[u] = *(const u32x2*)(vb + (int64_t)t * DH + lane * 4);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = t0 + u * 4;
      const float v0 = bflo(w[u][0]), v1 = bfhi(w[u][0]), v2 = bflo(w[u][1]), v3 = bfhi(w[u][1]);
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float pt = t < ctxs[q] ? sc[q * scld + t] : 0.f;
        acc[q][0] += pt * v0; acc[q][1] += pt * v1;
        acc[q][2] += pt * v2; acc[q][3] += pt * v3;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    *(f32x4*)(red + (wave * NQ + q) * DH + lane * 4) = (f32x4){acc[q][0], acc[q][1], acc[q][2], acc[q][3]};
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (ctxs[q] == 0) continue;                                  // a dead row's out row stays as it is
    const float inv = 1.0f / (wred[q * 8 + 4] + wred[q * 8 + 5] + wred[q * 8 + 6] + wred[q * 8 + 7]);
    const float v = (red[q * DH + tid] + red[(NQ + q) * DH + tid] + red[(2 * NQ + q) * DH + tid] + red[(3 * NQ + q) * DH + tid]) * inv;
    out[(int64_t)(b * NQ + q) * ld_out + (int64_t)h * DH + tid] = f2bf(v);
  }
}

// The refusals every decode-attention entry point has in common, stand-alone or co-launched (ap.rot_dim = 0 where the entry point
// has no rotary).  shared: pos_stride is left to attn_shared_check, which answers a wrong one in its own words.  also_null: a
// further pointer the entry point needs is missing.
static inline int attn_decode_check(const char* who, const AttnDecodeParams& ap, int32_t B, bool shared, bool also_null = false) {
  if (B <= 0 || ap.H <= 0 || ap.Smax <= 0 || ap.Smax > DEC_MAX_CTX) MG_FAIL(MG_ERR_SHAPE, "%s: need 0 < Smax <= %d", who, DEC_MAX_CTX);
  if (!shared && ap.pos_stride != 0 && ap.pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "%s: pos_stride must be 0 or 1", who);
  if (ap.rot_dim < 0 || ap.rot_dim > 256 || (ap.rot_dim & 7)) MG_FAIL(MG_ERR_SHAPE, "%s: rot_dim must be a multiple of 8 in [0,256]", who);
  if (!ap.qin || !ap.kcache || !ap.vcache || !ap.out || !ap.d_pos || also_null || (ap.rot_dim && (!ap.sin_t || !ap.cos_t)))
    MG_FAIL(MG_ERR_SHAPE, "%s: null pointer", who);
  if (!MG_ALIGNED16(ap.qin) || !MG_ALIGNED16(ap.kcache) || !MG_ALIGNED16(ap.vcache) || !MG_ALIGNED16(ap.out))
    MG_FAIL(MG_ERR_ALIGN, "%s: pointers must be 16-byte aligned", who);
  return MG_OK;
}

// The refusals of the chunk entry points, before any launch: attn_decode_check's in its words, then the chunk's own.
static inline int attn_chunk_check(const char* who, const AttnDecodeParams& ap, int32_t B, int32_t T) {
  if (int rc = attn_decode_check(who, ap, B, false)) return rc;
  if (T < 2 || T > DEC_CHUNK_MAX_Q) MG_FAIL(MG_ERR_SHAPE, "%s: need 2 <= T <= %d queries per sequence, got %d", who, DEC_CHUNK_MAX_Q, T);
  if ((int64_t)B * T > 16) MG_FAIL(MG_ERR_SHAPE, "%s: a chunk step serves at most 16 rows, got B * T = %d * %d", who, B, T);
  if (ap.ld_out != 0 && (ap.ld_out < (int64_t)ap.H * 256 || (ap.ld_out & 7))) MG_FAIL(MG_ERR_SHAPE, "%s: ld_out must be 0 or a multiple of 8 >= H*256", who);
  if (attn_chunk_lds_bytes(T, ap.Smax) > DEC_CHUNK_MAX_LDS)
    MG_FAIL(MG_ERR_SHAPE, "%s: T = %d queries over Smax = %d need %lld bytes of LDS, a workgroup has %d", who, T, ap.Smax,
            (long long)attn_chunk_lds_bytes(T, ap.Smax), DEC_CHUNK_MAX_LDS);
  return MG_OK;
}

// The refusals the shared-prefix entry points have in common (before any launch); fills `sh`.
static inline int attn_shared_check(const char* who, const AttnDecodeParams& ap, AttnSharedParams& sh, int32_t B, int32_t n_prefix,
                                    const float* part) {
  if (B > 16) MG_FAIL(MG_ERR_SHAPE, "%s: a shared prefix serves at most 16 rows, got B = %d", who, B);
  if (n_prefix < 1 || n_prefix > DEC_MAX_CTX) MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= n_prefix <= %d, got %d", who, DEC_MAX_CTX, n_prefix);
  if (ap.pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "%s: the rows of a shared prefix keep one position each (pos_stride must be 1)", who);
  if (!part) MG_FAIL(MG_ERR_SHAPE, "%s: null pointer", who);
  if (!MG_ALIGNED16(part)) MG_FAIL(MG_ERR_ALIGN, "%s: pointers must be 16-byte aligned", who);
  sh.n_prefix = n_prefix; sh.n_chunk = (n_prefix + PREFIX_CHUNK - 1) / PREFIX_CHUNK; sh.part = part;
  return MG_OK;
}
