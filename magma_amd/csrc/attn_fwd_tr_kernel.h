// attn_fwd_tr_kernel.h -- the text of the forward-attention kernel on V rows.  attention_tr.hip includes it three times, once per
// TRF_MODE (the comment there says what a mode changes); every other line is common to the three kernels.
#if TRF_MODE == TRF_TRAIN
__global__ __launch_bounds__(256) void attn_fwd32_tr_kernel(const AttnRows x, mg_bf16* __restrict__ out, int64_t ld_out,
                                                            float* __restrict__ lse, int B, int H, int S, float defer) {
#elif TRF_MODE == TRF_CACHED
// x.k / x.v = the layer's cache [B,H,Smax,256] as rows; the queries in c; S = T, the (padded) chunk length
__global__ __launch_bounds__(256) void attn_prefill_cached_tr_kernel(const AttnRows x, const AttnChunk c, mg_bf16* __restrict__ out,
                                                                     int64_t ld_out, int B, int H, int S, float defer) {
#else
__global__ __launch_bounds__(256) void attn_prefill_tree_tr_kernel(const AttnRows x, const AttnChunk c,
                                                                   const int* __restrict__ sub, mg_bf16* __restrict__ out,
                                                                   int64_t ld_out, int B, int H, int S, float defer) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int nblk = (S + 127) >> 7;
  const int wg = xcd_contiguous_index(blockIdx.x, gridDim.x);
  const int bh = wg / nblk, b = bh / H, h = bh - b * H;
  const int qt0 = (nblk - 1 - (wg - bh * nblk)) * 128;   // longest blocks first
  const int qrow = qt0 + wave * 32 + l31, qrow_c = min(qrow, S - 1);
  const int64_t xoff = (int64_t)b * x.stride_b + (int64_t)h * x.stride_h;
  const mg_bf16* kbase = x.k + xoff;
  const mg_bf16* vbase = x.v + xoff;
  const uint32_t ldb = (uint32_t)x.ld * 2u;
#if TRF_MODE == TRF_TRAIN
  const int klast = S - 1;                       // last key row a load may touch

  const int kv_end = min(S, qt0 + 128);
#else
  // d_pos is device-resident and never trusted: clamped into [0, Smax] before anything is derived from it (below 0 counts as 0,
  // above Smax as Smax -- a full cache; every key load then clamps to slot Smax - 1 and p + S <= 2 Smax cannot wrap)
  const int p = __builtin_amdgcn_readfirstlane(min(max(c.d_pos[(int64_t)b * c.pos_stride], 0), c.Smax));
  const int klast = min(p + S, c.Smax) - 1;      // last key row a load may touch

  const int kv_end = p + min(S, qt0 + 128);
#endif
  const int ntiles = (kv_end + 31) >> 5;
  const uint32_t smem_u = lds_u32(smem);
  const int row0 = wave * 8 + hi;
  const uint32_t c0b = (uint32_t)((l31 ^ ((hi << 2) | ((wave & 1) << 1))) << 4);
  // piece i (0..3) of the two images of tile min(t, last): past the last tile the ring re-loads it (in bounds, never read)
  auto issue_part = [&](int t, int buf, int i) {
    const int tc = min(t, ntiles - 1);
    const uint32_t st = smem_u + (uint32_t)(buf * TRF_STAGE + (wave * 4 + i) * 1024);
    const uint32_t off = (uint32_t)min(tc * 32 + row0 + 2 * i, klast) * ldb + (c0b ^ (uint32_t)((((i & 1) << 3) | (i >> 1)) << 4));
    glds16su(kbase, off, st);
    glds16su(vbase, off, st + ROW_TILE);
  };
  auto issue = [&](int t, int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) issue_part(t, buf, i);
  };
#pragma unroll
  for (int i = 0; i < TRF_STAGES - 1; ++i) issue(i, i);

  bf16x8 qf[16];
  {
#if TRF_MODE == TRF_TRAIN
    const mg_bf16* qp = x.q + xoff + (int64_t)qrow_c * x.ld + hi * 8;
#else
    const mg_bf16* qp = c.q + (int64_t)b * c.q_stride_b + (int64_t)h * c.q_stride_h + (int64_t)qrow_c * c.q_ld + hi * 8;
#endif
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
  }
  f32x16 o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = 0; j < 16; ++j) o[i][j] = 0.f;
  }
  float m2 = -1e30f, lsum = 0.f;
  const float sc2 = 0.0625f * 1.4426950408889634f;  // 1/sqrt(256) * log2(e)
  const int my_first = qt0 + wave * 32;
#if TRF_MODE == TRF_TRAIN
  const int n_act = min(ntiles, ((my_first + 31) >> 5) + 1);   // this wave's tiles: 0 .. n_act-1 (later ones are fully masked for it)
#else
  // this wave's tiles: 0 .. n_act-1 (later ones are fully masked for it).  A wave whose queries all lie past the chunk (T <= 96)
  // only feeds the ring: its rows are never stored
  const int n_act = my_first >= S ? 0 : min(ntiles, ((p + my_first + 31) >> 5) + 1);
#endif
  const int R = perm32(l31);
  const uint32_t rb = smem_u + row_base32(R, tr_swz(R), hi);
  const uint32_t tb0 = smem_u + tr_lane_base(lane);
  // key (r >> 3) 16 + (r & 7) of tile kv0 is visible iff it is <= lim0 - kv0
#if TRF_MODE == TRF_TRAIN
  const int lim0 = min(qrow, S - 1) - hi * 8;
#else
  const int lim0 = p + min(qrow, S - 1) - hi * 8;
#endif
#if TRF_MODE == TRF_TREE
  const int* subb = sub + (int64_t)b * S;             // ... and, a chunk key j, iff this query lies below sub[j]
#endif
  // ONE accumulator-file copy of the Q fragments (see attention_fwd32.hip)
  bf16x8 qa[16];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) asm volatile("" : "=a"(qa[ks]) : "0"(qf[ks]));

  bf16x8 fa[4], fb[4];
  f32x16 sA, sB;                       // scores of the current / the next tile, swapping roles every iteration (no copies)
  float alpha;
  auto part1 = [&](f32x16& sn, int kv0) {
#if TRF_MODE != TRF_TREE                               // causal: only the tiles on this wave's diagonal or past the last key
#if TRF_MODE == TRF_TRAIN
    if (kv0 + 31 > my_first || kv0 + 32 > S) {
#else
    if (kv0 + 31 > p + my_first || kv0 + 32 > p + S) {
#endif
      const int lim = lim0 - kv0;
#pragma unroll
      for (int r = 0; r < 16; ++r) sn[r] = ((r >> 3) * 16 + (r & 7)) > lim ? -1e30f : sn[r];
    }
#else
    if (kv0 + 32 > p) {                                // the tile reaches into the chunk (uniform over the wave)
      const int lim = lim0 - kv0;
      const int j = kv0 - p + l31;
      const int sj = subb[min(max(j, 0), S - 1)];
      const int sv = j < 0 ? 0x7fffffff : j >= S ? 0 : sj;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = (r >> 3) * 16 + (r & 7);
        const int s_lo = __builtin_amdgcn_readlane(sv, k), s_hi = __builtin_amdgcn_readlane(sv, k + 8);
        sn[r] = (k > lim || qrow_c >= (hi ? s_hi : s_lo)) ? -1e30f : sn[r];
      }
    }
#endif
    float tmax = sn[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, sn[r]);
    tmax = pair_max_tr(tmax);
    const float cand = tmax * sc2;
    const float mnew = (cand > m2 + defer) ? cand : m2;
    alpha = __builtin_amdgcn_exp2f(m2 - mnew);
    m2 = mnew;
  };

  // ---- prologue: tiles 0 and 1 landed; S^T(0) and part 1 of its softmax ----
  MG_WAIT_VMCNT(8);
  MG_BARRIER_KEEP_DMA();
  {
    rd_row4_asm(fa, rb, 0);
    rd_row4_asm(fb, rb, 1);
    MG_SCHED_FENCE();
    MG_LGKM(4);
    mfma32v0_ba(sA, fa[0], qa[0]);
#pragma unroll
    for (int i = 1; i < 4; ++i) mfma32v_ba(sA, fa[i], qa[i]);
    rd_row4_asm(fa, rb, 2);
    MG_SCHED_FENCE();
    MG_LGKM(4);
#pragma unroll
    for (int i = 0; i < 4; ++i) mfma32v_ba(sA, fb[i], qa[4 + i]);
    rd_row4_asm(fb, rb, 3);
    MG_SCHED_FENCE();
    MG_LGKM(4);
#pragma unroll
    for (int i = 0; i < 4; ++i) mfma32v_ba(sA, fa[i], qa[8 + i]);
    MG_SCHED_FENCE();
    MG_LGKM(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) mfma32v_ba(sA, fb[i], qa[12 + i]);
    mfma32v_ba_last(sA, fb[3], qa[15]);
    part1(sA, 0);
  }
  int sc = 0;
  // one iteration: `cur` = masked scores of tile t (part 1 done), `nxt` receives S^T(t+1)
  auto iteration = [&](f32x16& cur, f32x16& nxt, int t) {
    MG_WAIT_VMCNT(8);                 // this wave's pieces of tile t+1 landed (tile t+2 may be in flight)
    MG_BARRIER_KEEP_DMA();            // tile t+1 complete; everyone is done with iteration t-1 (K(t), V(t-1)); lgkmcnt = 0
    const int nb = sc == 0 ? TRF_STAGES - 1 : sc - 1;
    issue_part(t + TRF_STAGES - 1, nb, 0);
    issue_part(t + TRF_STAGES - 1, nb, 1);
    const int scn = sc == TRF_STAGES - 1 ? 0 : sc + 1;
    const uint32_t krow = (uint32_t)(scn * TRF_STAGE) + rb;
    const uint32_t tb = (uint32_t)(sc * TRF_STAGE) + tb0;
    float psum = 0.f, pe = 0.f;
    u32x4 pw0, pw1;
    auto soft = [&](int r) {          // element r of tile t (r even: kept for the pack with r + 1)
      const float pr = __builtin_amdgcn_exp2f(fmaf(cur[r], sc2, -m2));
      psum += pr;
      if (r & 1) { if (r < 8) pw0[r >> 1] = pack2bf(pe, pr); else pw1[(r - 8) >> 1] = pack2bf(pe, pr); }
      else pe = pr;
    };
    // ---- block A: S^T(t+1) MFMAs; behind each of them one exponential of tile t ----
    rd_row4_asm(fa, krow, 0);
    rd_row4_asm(fb, krow, 1);
    MG_SCHED_FENCE();
    MG_LGKM(4);                       // K0 | K1
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i == 0) mfma32v0_ba(nxt, fa[0], qa[0]); else mfma32v_ba(nxt, fa[i], qa[i]);
      MG_SCHED_FENCE();
      soft(i);
      MG_SCHED_FENCE();
    }
    rd_row4_asm(fa, krow, 2);
    MG_SCHED_FENCE();
    MG_LGKM(4);                       // K1 | K2
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mfma32v_ba(nxt, fb[i], qa[4 + i]);
      MG_SCHED_FENCE();
      soft(4 + i);
      MG_SCHED_FENCE();
    }
    rd_row4_asm(fb, krow, 3);
    MG_SCHED_FENCE();
    MG_LGKM(4);                       // K2 | K3
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mfma32v_ba(nxt, fa[i], qa[8 + i]);
      MG_SCHED_FENCE();
      soft(8 + i);
      MG_SCHED_FENCE();
    }
    rd_t_half<ROW_TILE, 0>(fa[0], fa[1], tb);      // V^T halves of tile t through the ring {fa[0..1], fa[2..3], fb[0..1], fb[2..3]}
    rd_t_half<ROW_TILE, 1>(fa[2], fa[3], tb);
    MG_SCHED_FENCE();
    MG_LGKM(8);                       // K3 | T0, T1
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < 3) mfma32v_ba(nxt, fb[i], qa[12 + i]); else mfma32v_ba_last(nxt, fb[3], qa[15]);
      MG_SCHED_FENCE();
      soft(12 + i);
      MG_SCHED_FENCE();
    }
    rd_t_half<ROW_TILE, 2>(fb[0], fb[1], tb);
    lsum = lsum * alpha + psum;
    bf16x8 pf0 = __builtin_bit_cast(bf16x8, pw0), pf1 = __builtin_bit_cast(bf16x8, pw1);
    mfma_operand_ready(pf0, pf1);
    MG_SCHED_FENCE();
    issue_part(t + TRF_STAGES - 1, nb, 2);
    issue_part(t + TRF_STAGES - 1, nb, 3);
    // ---- the running maximum moved by more than the deferral threshold (rare): O^T and l were kept at the old one ----
    if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
      asm volatile("" : "+a"(o[0]), "+a"(o[1]), "+a"(o[2]), "+a"(o[3]), "+a"(o[4]), "+a"(o[5]), "+a"(o[6]), "+a"(o[7]));
#pragma unroll
      for (int db = 0; db < 8; ++db) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
        asm volatile("" : "+a"(o[db]));      // back in its AGPRs before the next tuple is touched
        MG_SCHED_FENCE();
      }
    }
    MG_SCHED_FENCE();
    // ---- block B: O^T += V^T(t) P^T(t), 16 MFMAs = 8 halves; part 1 of softmax(t+1) behind the first two ----
    MG_LGKM(8);                       // T0 | T1, T2
    mfma32a(o[0], fa[0], pf0); mfma32a(o[1], fa[1], pf0);
    rd_t_half<ROW_TILE, 3>(fb[2], fb[3], tb);
    MG_SCHED_FENCE();
    MG_LGKM(8);                       // T1 | T2, T3
    mfma32a(o[0], fa[2], pf1); mfma32a(o[1], fa[3], pf1);
    rd_t_half<ROW_TILE, 4>(fa[0], fa[1], tb);
    MG_SCHED_FENCE();
    part1(nxt, (t + 1) * 32);
    MG_SCHED_FENCE();
    MG_LGKM(8);                       // T2 | T3, T4
    mfma32a(o[2], fb[0], pf0); mfma32a(o[3], fb[1], pf0);
    rd_t_half<ROW_TILE, 5>(fa[2], fa[3], tb);
    MG_SCHED_FENCE();
    MG_LGKM(8);                       // T3 | T4, T5
    mfma32a(o[2], fb[2], pf1); mfma32a(o[3], fb[3], pf1);
    rd_t_half<ROW_TILE, 6>(fb[0], fb[1], tb);
    MG_SCHED_FENCE();
    MG_LGKM(8);                       // T4 | T5, T6
    mfma32a(o[4], fa[0], pf0); mfma32a(o[5], fa[1], pf0);
    rd_t_half<ROW_TILE, 7>(fb[2], fb[3], tb);
    MG_SCHED_FENCE();
    MG_LGKM(8);                       // T5 | T6, T7
    mfma32a(o[4], fa[2], pf1); mfma32a(o[5], fa[3], pf1);
    MG_SCHED_FENCE();
    MG_LGKM(4);                       // T6 | T7
    mfma32a(o[6], fb[0], pf0); mfma32a(o[7], fb[1], pf0);
    MG_SCHED_FENCE();
    MG_LGKM(0);                       // T7
    mfma32a(o[6], fb[2], pf1);
    mfma32a_last(o[7], fb[3], pf1);
    sc = scn;
  };
  int t = 0;
  for (; t + 1 < n_act; t += 2) {
    iteration(sA, sB, t);
    iteration(sB, sA, t + 1);
  }
  if (t < n_act) { iteration(sA, sB, t); ++t; }
  for (; t < ntiles; ++t) {           // tiles that only the later waves of the block need: move this wave's share of them
    MG_WAIT_VMCNT(8);
    MG_BARRIER_KEEP_DMA();
    issue(t + TRF_STAGES - 1, sc == 0 ? TRF_STAGES - 1 : sc - 1);
    sc = sc == TRF_STAGES - 1 ? 0 : sc + 1;
  }
  MG_WAIT_VMCNT(0);                   // drain the ring's trailing loads before the ring becomes staging space
  MG_BARRIER_KEEP_DMA();
  lsum = pair_sum_tr(lsum);
  const float inv = 1.0f / lsum;
  // O^T (acc[db] = d-rows db*32.. x 32 queries) -> bf16 rows through a wave-private LDS image, out as whole 512-byte rows
  char* stage = smem + wave * (32 * EP_ROW);
  char* wr = stage + l31 * EP_ROW + hi * 8;
#pragma unroll
  for (int db = 0; db < 8; ++db) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const u32x2 w = {pack2bf(o[db][rq * 4] * inv, o[db][rq * 4 + 1] * inv), pack2bf(o[db][rq * 4 + 2] * inv, o[db][rq * 4 + 3] * inv)};
      *(u32x2*)(wr + db * 64 + rq * 16) = w;
    }
    MG_SCHED_FENCE();             // one tuple at a time: 128 accumulators read at once are 128 VGPRs the loop pays for
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int row = it * 2 + hi;
    const u32x4 w = *(const u32x4*)(stage + row * EP_ROW + l31 * 16);
    const int s = qt0 + wave * 32 + row;
    if (s < S) *(u32x4*)(out + (int64_t)(b * S + s) * ld_out + h * DH + l31 * 8) = w;
  }
#if TRF_MODE == TRF_TRAIN
  if (lse && hi == 0 && qrow < S) lse[(int64_t)bh * S + qrow] = (m2 + log2f(lsum)) * 0.6931471805599453f;
#endif
}
