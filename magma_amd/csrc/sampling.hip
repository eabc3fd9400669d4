// sampling.hip -- the non-greedy branch of the decode loop on the device:
// reference magma/sampling.py:99-107
//     if top_k > 0: logits = top_k_filter(logits, k=top_k)          (:22-30)
//     if top_p > 0: logits = top_p_filter(logits, threshold=top_p)  (:7-19, the reference's own rule -- SURVEY Q6)
//     probs = softmax(logits / temperature); next_token = multinomial(probs, 1)
// and the early-stop test (next_token == eos).all() (:109), as ONE launch per token step + a one-thread bookkeeping
// launch, both graph-capturable: no host round trip per step (the reference syncs once per token, and runs the filters
// as ~10 PyTorch launches including a full sort of the 50 258 logits).
//
// One workgroup of 1024 threads per row; the row (200 KB of fp32 at V = 50 258) stays in L2 and is swept a few times:
//   top-k        threshold = the k-th largest logit by MSB-first radix selection on order-preserving 32-bit keys
//                (4 sweeps, integer histograms in LDS); every logit below it becomes -inf; of the ties AT the threshold the
//                first ones by index stay, so that exactly k survive (torch.topk keeps an unspecified subset of them --
//                equal values, so the probability mass the next stage sees is the same).
//   "top-p"      the reference sorts descending, accumulates softmax probabilities and DROPS every rank r >= 1 whose
//                preceding mass cum[r-1] is still below 1 - threshold.  No sort is needed for that: an element is dropped
//                iff it is not the first maximum and the probability mass of the strictly larger logits is < 1 - threshold,
//                and that mass is monotone in the logit -- so the set is {x >= t*} minus the maximum, with t* the smallest
//                logit whose strictly-larger mass is below the bound.  t* comes from the same radix descent with MASS
//                histograms, preceded (round 3) by one level of 256 LINEAR value bins over [max(min, max - 32), max]: the
//                key's top byte puts nearly all 50 258 logits into two or three buckets -- one LDS atomic queue -- and a
//                monotone partition of any shape keeps the descent's invariant; the 256 buckets of a level are scanned by
//                one wave (suffix sums by shuffles, the monotone predicate by ballot) instead of one thread.  172 -> ~120 us
//                per step for 8 rows.  Masses are 2^-40 fixed point in 64-bit integers: integer atomics are associative, so the
//                result does not depend on the order in which the lanes arrive (fp32 atomics would make a sampled token
//                depend on scheduling).  Ties at t* are dropped one by one in index order, as a stable sort would.
//   multinomial  inverse-CDF draw in index order over the same fixed-point weights exp((x - max) / temperature):
//                target = floor(r * total / 2^64) with r = 64 Philox4x32-10 bits keyed by (seed, step, row); prefix sums
//                are integer, hence exact and reproducible (tests restate the draw in Python integers / float64).
//
// transformers' sampler (mg_sample_warp_f32; DESIGN.md "transformers' sampler"; host statements: sampling.py top_k_filter_ties,
// nucleus_filter, min_p_filter) is the same body compiled with WARP = true -- the rules of TemperatureLogitsWarper, TopKLogitsWarper,
// TopPLogitsWarper and MinPLogitsWarper with min_tokens_to_keep = 1, then the same draw:
//   top-k        every tie at the k-th value stays (no index cut).
//   top-p        masses at temperature T over the top-k survivors; a token stays iff the mass ranked before it is below
//                total - (1 - top_p): the same descent with limit = total - c instead of c (total = the sum of the level-0
//                histogram), the kept set is {key >= t*} instead of "dropped = {key >= t*} minus the maximum", the first ties at t*
//                by index stay.  The level-0 bins span [max(min, max - 32 T), max].
//   min-p        a token stays iff x >= max + T log(min_p): one more comparison in `kept`, no sweep.
// The instance with WARP = false is the kernel as it was.
//
// Per-request sampling (mg_sample_rows_f32; DESIGN.md "Per-request sampling"): both instances once more with S = TableRows -- the
// same body, every workgroup taking its scalars and seed from its row's record of a device table and drawing at the counter
// (the row's own token index, 0), which is what row 0 of a one-row flat call draws at.  S = FlatRows is the kernel as it was.
//
// Speculative decoding for sampled rows (mg_sample_chunk_f32; DESIGN.md "Speculative decoding"): both instances a third time with
// S = ChunkRows -- one workgroup per fed row b * T + t of a speculative step, the record of SEQUENCE b, the draw at the counter
// (count[b] + t, 0): the index the row's token has in b's own stream when the drafts in front of it were right, which is the only
// case spec_finish_kernel keeps it in.  The rows that kernel never reads are skipped whole.
#include "common.h"
#include <type_traits>

namespace {

constexpr int ST = 1024;

MG_DEV uint32_t fkey(float x) {            // order-preserving map float -> uint32 (larger float, larger key)
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ---- deterministic block reductions (fixed tree, 16 waves) ----
MG_DEV float blk_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int w = 1; w < ST / 64; ++w) r = fmaxf(r, sh[w]);
  return r;
}
MG_DEV float blk_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int w = 1; w < ST / 64; ++w) r += sh[w];
  return r;
}
MG_DEV int blk_min_i(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = sh[0];
#pragma unroll
  for (int w = 1; w < ST / 64; ++w) r = min(r, sh[w]);
  return r;
}

// Philox4x32-10 (Salmon et al. 2011), counter (c0..c3), key (k0, k1)
MG_DEV void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

struct SampleParams {
  const float* logits; int64_t ld; int V;
  float temperature; int top_k; double top_p;
  const uint64_t* seed;       // device: 64-bit seed (may change between graph replays)
  const int32_t* state;       // device: [0] = step counter (read here, advanced by sample_finish_kernel)
  int64_t* out;               // [B] sampled token (nullptr: filter only)
  float* filtered; int64_t ldf;   // optional [B, V] filtered logits (tests / callers that want the reference's tensor)
};

struct WarpParams : SampleParams {
  double log_min_p;           // log(min_p), -inf when min-p is off
};

constexpr double FIX = 1099511627776.0;   // 2^40

// The window of row b of a slot session before this step's selection, from the tables mg_sample_finish_slots keeps
// (slot[b] = {begin, limit}, finish[b] = {step or -1, code}) and s = state[0]: the occupant's n = ((s - 1) % cols - begin) mod
// cols + 1 tokens from column begin on -- the count sample_finish_slots_kernel forms.  n = 0: the row is idle (finished and not
// harvested yet, or never occupied) or its begin lies outside the ring; such a row is skipped whole.  s is any value: the
// column is formed as slots_admit_kernel forms it, and n lies in [1, cols] by construction.
struct SlotWin { int begin, n; };
MG_DEV SlotWin slot_window(const int32_t* __restrict__ state, const int32_t* __restrict__ slot, const int32_t* __restrict__ finish,
                           int b, int cols) {
  if (finish[2 * (int64_t)b] >= 0) return SlotWin{0, 0};
  const int begin = slot[2 * (int64_t)b];
  if (begin < 0 || begin >= cols) return SlotWin{0, 0};
  const int prev = (int)((unsigned)state[0] - 1u);
  const int col = ((prev % cols) + cols) % cols;
  int d = col - begin;                      // in (-cols, cols)
  if (d < 0) d += cols;
  return SlotWin{begin, d + 1};
}

// Where a workgroup takes its scalars from (DESIGN.md "Per-request sampling").  FlatRows: the launch arguments, one set for all
// rows, the draw at counter (state[0], row) under *seed -- mg_sample_f32 / mg_sample_warp_f32 as they were.  TableRows
// (mg_sample_rows_f32): row r's record of a device table, read at run time, and the draw at counter (j, 0) under the record's seed,
// with j the row's own token index -- state[0] of a static call, or the occupant's token count so far from the slot session's
// tables (slot_window's n: sample_finish_slots_kernel's n - 1 for the token this step selects).  Those are the key and the counter
// of row 0 of a one-row flat call at step j.
struct FlatRows {};
struct SampleRow {            // MG_SAMPLE_ROW_BYTES = 32, 16-byte aligned
  double top_p;
  double log_min_p;           // log(min_p) as mg_sample_warp_f32 forms it on the host, -inf: off (read by the WARP instance only)
  uint64_t seed;
  float temperature;          // 0 (or anything that is not a finite value > 0): the row is greedy
  int32_t top_k;              // <= 0 or >= V: off
};
static_assert(sizeof(SampleRow) == MG_SAMPLE_ROW_BYTES, "the record of mg_sample_rows_f32");
struct TableRows { const SampleRow* rows; const int32_t* slot; const int32_t* finish; int hist_cols; };
// ChunkRows (mg_sample_chunk_f32; DESIGN.md "Speculative decoding"): the selection of a speculative step that fed T rows per
// sequence.  Workgroup r = b * T + t takes the record of SEQUENCE b and draws at counter (count[b] + t, 0) -- the index the token
// would have in b's own stream if every draft in front of it was right, which is the only case spec_finish_kernel keeps it in.
// count is that kernel's count, read before it moves.  The rows it never reads are skipped whole.
struct ChunkRows { const SampleRow* rows; const int32_t* count; const int32_t* n_draft; const int32_t* finish; int hist_cols, T; };

struct RowScalars { float temperature; int top_k; double top_p, log_min_p; };

template <class P, class S = FlatRows>
__global__ __launch_bounds__(ST) void sample_kernel(const P p0, const S src) {
  constexpr bool WARP = std::is_same<P, WarpParams>::value;
  constexpr bool CHUNK = std::is_same<S, ChunkRows>::value;
  constexpr bool ROWS = std::is_same<S, TableRows>::value || CHUNK;
  // `p`: the row's scalars under the names the body reads -- the launch arguments, or the row's record
  RowScalars p{p0.temperature, p0.top_k, p0.top_p, -(double)INFINITY};
  if constexpr (WARP) p.log_min_p = p0.log_min_p;
  uint32_t ctr0 = 0u, ctr1 = blockIdx.x;
  unsigned long long seed = 0ull;
  bool greedy = false;
  if constexpr (ROWS) {
    int rec = blockIdx.x;
    if constexpr (CHUNK) {      // a speculative step: the rows spec_finish_kernel never reads are skipped whole (uniform)
      const int b = blockIdx.x / src.T, t = blockIdx.x % src.T;
      const int c = src.count[b];
      if (src.finish[2 * (int64_t)b] >= 0 || c < 0 || c > src.hist_cols) return;
      const int nd = src.n_draft ? max(0, min(src.n_draft[b], src.T - 1)) : 0;
      if (t > nd) return;
      ctr0 = (uint32_t)(c + t);
      rec = b;
    } else if (src.slot) {      // a slot session: idle rows are skipped whole (uniform over the workgroup)
      const SlotWin w = slot_window(p0.state, src.slot, src.finish, blockIdx.x, src.hist_cols);
      if (w.n == 0) return;
      ctr0 = (uint32_t)w.n;
    } else {
      ctr0 = (uint32_t)p0.state[0];
    }
    ctr1 = 0u;
    const SampleRow r = src.rows[rec];
    // the table is device memory no entry point can look at: a temperature that is not a finite value > 0 selects greedily, a
    // negative top_k is off (nothing below forms an address from a record's value)
    greedy = !(r.temperature > 0.f) || r.temperature == INFINITY;
    p.temperature = greedy ? 1.0f : r.temperature;
    p.top_k = greedy || r.top_k < 0 ? 0 : r.top_k;
    p.top_p = greedy ? 0.0 : r.top_p;
    p.log_min_p = greedy || !WARP ? -(double)INFINITY : r.log_min_p;
    seed = r.seed;
  } else {
    if (p0.out) { ctr0 = (uint32_t)p0.state[0]; seed = p0.seed ? *p0.seed : 0ull; }
  }
  __shared__ unsigned long long hist64[256];
  __shared__ uint32_t hist32[256];
  __shared__ float shf[ST / 64];
  __shared__ int shi[ST / 64];
  __shared__ unsigned long long shu[ST / 64 + 1];
  __shared__ uint32_t bc[4];
  __shared__ unsigned long long bc64[2];
  const int tid = threadIdx.x, V = p0.V;
  const float* x = p0.logits + (int64_t)blockIdx.x * p0.ld;

  // One wave scans the 256 buckets of a top-p level (it used to be one thread walking them: ~8 us per level): the lowest
  // non-empty bucket whose strictly-larger mass -- `start` plus the buckets above it -- is below `limit`.  That mass only grows
  // downwards, so the predicate is monotone: suffix sums by shuffles, the lowest qualifying bucket by ballot.
  auto scan_mass = [&](unsigned long long start, unsigned long long limit) {
    if (tid < 64) {
      unsigned long long m[4]; uint32_t c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { m[j] = hist64[4 * tid + j]; c[j] = hist32[4 * tid + j]; }
      const unsigned long long lane_sum = m[0] + m[1] + m[2] + m[3];
      unsigned long long incl = lane_sum;                   // sum over lanes >= this one
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_down(incl, o, 64);
        if (tid + o < 64) incl += t;
      }
      const unsigned long long s3 = start + (incl - lane_sum);    // mass strictly above bucket 4 * tid + 3
      const unsigned long long s2 = s3 + m[3], s1 = s2 + m[2], s0 = s1 + m[1];
      int j = -1; unsigned long long sj = 0;
      if (c[0] && s0 < limit) { j = 0; sj = s0; }
      else if (c[1] && s1 < limit) { j = 1; sj = s1; }
      else if (c[2] && s2 < limit) { j = 2; sj = s2; }
      else if (c[3] && s3 < limit) { j = 3; sj = s3; }
      const unsigned long long has = __ballot(j >= 0);
      if (has == 0ull) { if (tid == 0) { bc[0] = 0u; bc[1] = 0u; bc64[0] = start; bc64[1] = 0ull; } }
      else if (tid == (int)__builtin_ctzll(has)) { bc[0] = (uint32_t)(4 * tid + j); bc[1] = c[j]; bc64[0] = sj; bc64[1] = m[j]; }
    }
  };

  // ---------------- top-k: key of the k-th largest logit ----------------
  uint32_t tk = 0;                                  // alive(i) = key > tk || (key == tk && i < k_cut): exactly k survive
  int k_cut = 0x7fffffff;
  if (p.top_k > 0 && p.top_k < V) {
    uint32_t prefix = 0, mask = 0, remaining = (uint32_t)p.top_k;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist32[tid] = 0;
      __syncthreads();
      for (int i = tid; i < V; i += ST) {
        const uint32_t k = fkey(x[i]);
        if ((k & mask) == prefix) atomicAdd(&hist32[(k >> shift) & 255], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t rem = remaining; int d = 0;
        for (int b = 255; b >= 0; --b) {
          if (hist32[b] >= rem) { d = b; break; }
          rem -= hist32[b];
        }
        bc[0] = (uint32_t)d; bc[1] = rem; bc[2] = hist32[d];
      }
      __syncthreads();
      prefix |= bc[0] << shift; mask |= 255u << shift; remaining = bc[1];
      const uint32_t in_bucket = bc[2];
      __syncthreads();
      if (shift == 0 && in_bucket > remaining && !WARP) {     // more ties at the threshold than places left: the first ones by index stay
        if (tid == 0) {
          uint32_t seen = 0; int cut = 0x7fffffff;
          for (int i = 0; i < V; ++i) if (fkey(x[i]) == prefix) { if (seen == remaining) { cut = i; break; } ++seen; }
          bc[3] = (uint32_t)cut;
        }
        __syncthreads();
        k_cut = (int)bc[3];
        __syncthreads();
      }
    }
    tk = prefix;
  }
  auto alive = [&](int i, uint32_t k) -> bool { return k > tk || (k == tk && i < k_cut); };      // WARP: k >= tk, every tie stays

  // ---------------- first maximum (rank 0 of the reference's sort; never dropped) ----------------
  float mx = -INFINITY, mn = INFINITY;      // mn: smallest finite logit (only spans the top-p level-0 bins)
  for (int i = tid; i < V; i += ST) { const float v = x[i]; mx = fmaxf(mx, v); if (v > -INFINITY) mn = fminf(mn, v); }
  mx = blk_max(mx, shf);
  mn = -blk_max(-mn, shf);
  int imax = 0x7fffffff;
  for (int i = tid; i < V; i += ST) if (x[i] == mx) { imax = min(imax, i); }
  imax = blk_min_i(imax, shi);
  if constexpr (ROWS) {
    if (greedy) {             // a temperature-0 row of the table: the first maximum, as mg_argmax_f32 (uniform over the workgroup)
      if (p0.filtered) {
        float* f = p0.filtered + (int64_t)blockIdx.x * p0.ldf;
        for (int i = tid; i < V; i += ST) f[i] = i == imax ? x[i] : -INFINITY;
      }
      if (p0.out && tid == 0) p0.out[blockIdx.x] = imax == 0x7fffffff ? 0 : imax;
      return;
    }
  }

  // ---------------- the reference's top-p rule ----------------
  uint32_t tstar = WARP ? 0u : 0xffffffffu;    // dropped(i) = alive && i != imax && (key > tstar || (key == tstar && i < tie_cut))
  int tie_cut = WARP ? 0x7fffffff : 0;         // WARP: kept(i) = alive && (key > tstar || (key == tstar && i < tie_cut)) && x >= min-p bound
  // the reference compares an fp32 tensor with the PYTHON scalar (1 - threshold): the scalar is evaluated in double, then cast
  // to fp32 for the comparison -- top_p arrives as a double so that exactly that value is formed (0.1f for 0.9, not 0.10000002f)
  const double bound = (double)(float)(1.0 - p.top_p);
  if (p.top_p > 0.0 && bound > 0.0) {
    const float rtp = 1.0f / p.temperature;
    auto mass = [&](float v) -> float {      // WARP: the probabilities the nucleus is cut from are those at temperature T
      if constexpr (WARP) return __expf((v - mx) * rtp);
      else return __expf(v - mx);
    };
    float z = 0.f;
    for (int i = tid; i < V; i += ST) if (alive(i, fkey(x[i]))) z += mass(x[i]);
    z = blk_sum(z, shf);
    const float rz = 1.0f / z;
    unsigned long long cfix = (unsigned long long)(bound * FIX);      // WARP: becomes total - c once level 0 is summed
    // Level 0: 256 LINEAR value bins over [max(min, max - 32), max] (below max - 32 the fixed-point mass is 0), then the four 8-bit levels of
    // the order-preserving key inside the chosen bin.  Any monotone partition keeps the descent's invariant (`above` = mass
    // strictly above the current range), so t* is what four key levels alone would find -- but the key's top byte (sign + high
    // exponent bits) puts nearly all of the 50 000 logits into two or three buckets, i.e. one LDS atomic queue; linear bins
    // spread them.
    const float lo = fmaxf(mn, WARP ? mx - 32.0f * p.temperature : mx - 32.0f);
    const float bscale = mx > lo ? 255.99f / (mx - lo) : 0.f;
    auto bin0 = [&](float v) -> int { const int b = (int)((v - lo) * bscale); return v > lo ? min(b, 255) : 0; };
    uint32_t prefix = 0, mask = 0;
    unsigned long long above = 0;     // mass of the alive keys strictly above the current range
    uint32_t n_eq = 0;
    int b0 = 0;
    for (int level = 0; level < 5; ++level) {
      const int shift = 24 - 8 * (level - 1);            // levels 1..4: key bytes, most significant first
      if (tid < 256) { hist64[tid] = 0; hist32[tid] = 0; }
      __syncthreads();
      for (int i = tid; i < V; i += ST) {
        const float v = x[i];
        const uint32_t k = fkey(v);
        if (alive(i, k)) {
          const int vb = bin0(v);
          if (level == 0 || (vb == b0 && (k & mask) == prefix)) {
            const int bucket = level == 0 ? vb : (int)((k >> shift) & 255);
            const unsigned long long q = (unsigned long long)((double)(mass(v) * rz) * FIX + 0.5);
            atomicAdd(&hist64[bucket], q);
            atomicAdd(&hist32[bucket], 1u);
          }
        }
      }
      __syncthreads();
      if constexpr (WARP) {
        if (level == 0) {      // limit = total - c, at least 1 so that the first maximum (preceding mass 0) always stays
          if (tid < 64) {
            unsigned long long t = hist64[4 * tid] + hist64[4 * tid + 1] + hist64[4 * tid + 2] + hist64[4 * tid + 3];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
            if (tid == 0) bc64[0] = t;
          }
          __syncthreads();
          const unsigned long long total = bc64[0];
          cfix = total > cfix ? total - cfix : 1ull;
          __syncthreads();
        }
      }
      scan_mass(above, cfix);
      __syncthreads();
      if (level == 0) b0 = (int)bc[0];
      else { prefix |= bc[0] << shift; mask |= 255u << shift; n_eq = bc[1]; }
      above = bc64[0];
      __syncthreads();
    }
    tstar = prefix;
    // ties at t*: the j-th of them (index order) has preceding mass above + j * q_eq
    int m = (int)n_eq;
    if (n_eq > 1) {
      const unsigned long long q_eq = bc64[1] / n_eq;
      unsigned long long s = above; m = 0;
      while (m < (int)n_eq && s < cfix) { ++m; s += q_eq; }
    }
    tie_cut = 0x7fffffff;
    if (m < (int)n_eq) {           // rare: only the first m ties (by index) go (WARP: stay) -- one thread finds the (m+1)-th tie's index
      if (tid == 0) {
        int seen = 0, cut = 0x7fffffff;
        for (int i = 0; i < V; ++i) if (fkey(x[i]) == tstar && alive(i, tstar)) { if (seen == m) { cut = i; break; } ++seen; }
        bc[2] = (uint32_t)cut;
      }
      __syncthreads();
      tie_cut = (int)bc[2];
    }
  }
  float minp_bound = -INFINITY;      // WARP: the smallest fp32 that is >= max + T log(min_p)
  if constexpr (WARP) {
    if (p.log_min_p > -INFINITY) {
      const double t = (double)mx + (double)p.temperature * p.log_min_p;
      minp_bound = (float)t;
      if ((double)minp_bound < t) minp_bound = nextafterf(minp_bound, INFINITY);
    }
  }
  auto kept = [&](int i, float v) -> bool {
    const uint32_t k = fkey(v);
    if (!alive(i, k)) return false;
    if (i == imax) return true;
    if constexpr (WARP) return (k > tstar || (k == tstar && i < tie_cut)) && v >= minp_bound;
    else return !(k > tstar || (k == tstar && i < tie_cut));
  };

  if (p0.filtered) {
    float* f = p0.filtered + (int64_t)blockIdx.x * p0.ldf;
    for (int i = tid; i < V; i += ST) { const float v = x[i]; f[i] = kept(i, v) ? v : -INFINITY; }
  }
  if (!p0.out) return;

  // ---------------- multinomial draw: inverse CDF over fixed-point weights, index order ----------------
  // Wave w owns the contiguous index range [w * RW * 64, (w + 1) * RW * 64) as RW rows of 64: lane l reads index
  // seg0 + j * 64 + l, so every load is one coalesced 256-byte row (a contiguous range PER THREAD made each load instruction
  // touch 64 cache lines).  Index order inside the range is (row, lane): the wave that holds the target walks its rows with a
  // lane scan per row.  Same integers, same order of the CDF: the same token as before.
  const int lane = tid & 63, wave = tid >> 6;
  const int RW = (V + ST - 1) / ST;
  const int seg0 = wave * RW * 64;
  const float rt = 1.0f / p.temperature;
  auto weight = [&](int i) -> unsigned long long {
    if (i >= V) return 0ull;
    const float v = x[i];
    return kept(i, v) ? (unsigned long long)((double)__expf((v - mx) * rt) * 4294967296.0 + 0.5) : 0ull;
  };
  unsigned long long wsum = 0;
  for (int j = 0; j < RW; ++j) wsum += weight(seg0 + j * 64 + lane);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wsum += __shfl_xor(wsum, o, 64);          // total of this wave's range, in every lane
  __syncthreads();
  if (lane == 0) shu[wave] = wsum;
  __syncthreads();
  if (tid == 0) {
    unsigned long long run = 0;
    for (int w = 0; w < ST / 64; ++w) { const unsigned long long t = shu[w]; shu[w] = run; run += t; }
    shu[ST / 64] = run;
  }
  __syncthreads();
  const unsigned long long excl = shu[wave], total = shu[ST / 64];
  uint32_t c[4] = {ctr0, ctr1, 0u, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const unsigned long long r = ((unsigned long long)c[0] << 32) | c[1];
  const unsigned long long target = __umul64hi(r, total);           // uniform in [0, total)
  if (wsum > 0 && target >= excl && target < excl + wsum) {         // exactly one wave (the condition is wave-uniform)
    unsigned long long run = excl;
    for (int j = 0; j < RW; ++j) {
      const int i = seg0 + j * 64 + lane;
      unsigned long long incl = weight(i);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      const unsigned long long row_total = __shfl(incl, 63, 64);
      if (run + row_total > target) {                               // the token is in this row
        const unsigned long long hit = __ballot(run + incl > target);
        if (lane == 0) p0.out[blockIdx.x] = seg0 + j * 64 + (int)__builtin_ctzll(hit);     // first index whose inclusive CDF exceeds the target
        break;
      }
      run += row_total;
    }
  }
  if (total == 0 && tid == 0) p0.out[blockIdx.x] = imax == 0x7fffffff ? 0 : imax;   // nothing representable: the maximum
}

// Loop bookkeeping of one token step in ONE small launch: (next_token == eos).all() of reference sampling.py:109 recorded as
// the FIRST step at which it held, the step counter of the random stream, the KV-cache write position, and the token
// history the host reads once at the end of generate() (instead of one small copy per step).  n_pos = 1 (one position for
// the batch) or B (one per row of a ragged batch): every entry advances by delta.
// state = {step, first_all_eos_step (-1 = not yet)}
__global__ void sample_finish_kernel(const int64_t* __restrict__ tok, int B, int64_t eos, int32_t* __restrict__ state,
                                     int32_t* __restrict__ d_pos, int delta, int n_pos, int64_t* __restrict__ history, int64_t ld_hist,
                                     int hist_cols, int32_t* __restrict__ clear, int n_clear, int clear_stride) {
  // every thread needs the step BEFORE thread 0 bumps it: one read, broadcast through LDS (rows beyond the first wave would
  // otherwise race with the increment below)
  __shared__ int s_step;
  if (threadIdx.x == 0) s_step = state[0];
  __syncthreads();
  const int step = s_step;
  for (int i = threadIdx.x; i < n_clear; i += blockDim.x) clear[(int64_t)i * clear_stride] = 0;
  if (history && step >= 0 && step < hist_cols)        // (the step is device-resident: outside the history nothing is written)
    for (int b = threadIdx.x; b < B; b += blockDim.x) history[(int64_t)b * ld_hist + step] = tok[b];
  if (d_pos)
    for (int b = threadIdx.x; b < n_pos; b += blockDim.x) d_pos[b] += delta;
  if (threadIdx.x != 0) return;
  bool all = true;
  for (int b = 0; b < B; ++b) all = all && (tok[b] == eos);
  if (all && state[1] < 0) state[1] = step;
  state[0] = step + 1;
}

// The row test of per-row stopping, shared by sample_finish_rows_kernel, sample_finish_slots_kernel and slots_admit_kernel: the
// code the row finishes with at token t, or 0.  t is the row's newest token, already written at column `col` of its history h; n is
// the number of the row's OWN tokens up to and including t, so a sequence longer than n cannot match and no older column is read;
// a column index below 0 wraps by `cols` (a ring history; the plain history has n <= col + 1 and never wraps).  eos is tested first.
__device__ __forceinline__ int stop_row_code(int64_t t, const int64_t* __restrict__ h, int col, int n, int cols,
                                             const int32_t* __restrict__ table, int n_eos, int n_seq, bool seqs) {
  const int32_t* seq_len = table + MG_STOP_MAX_EOS;
  const int32_t* seq_tok = seq_len + MG_STOP_MAX_SEQ;
  int code = 0;
  for (int e = 0; e < n_eos && !code; ++e)
    if (t == (int64_t)table[e]) code = MG_STOP_EOS | e;
  if (!code && seqs) {
    for (int s = 0; s < n_seq && !code; ++s) {
      const int L = seq_len[s];
      if (L < 1 || L > MG_STOP_MAX_LEN || L > n) continue;
      bool eq = true;
      for (int j = 0; j < L; ++j) {
        int c = col - L + 1 + j;
        if (c < 0) c += cols;
        eq = eq && h[c] == (int64_t)seq_tok[s * MG_STOP_MAX_LEN + j];
      }
      if (eq) code = MG_STOP_SEQ | s;
    }
  }
  return code;
}

// Per-row stopping (DESIGN.md "Per-row stopping"; host statement: sampling.py stop_update): the bookkeeping above with the rule of
// transformers' _sample -- a finished row is padded and stays finished, the loop ends when no row is unfinished -- for up to 8 eos
// ids and 16 stop sequences of up to 16 tokens, read from a device table (its contents may change between graph replays, the
// counts are launch arguments).  Still one workgroup: rows are strided over it, every row is handled by one thread (its history
// write and its tail reads are that thread's own), and the "some row is unfinished" flag goes through LDS with a barrier
// between the row loop and thread 0's read, so B may exceed the workgroup.
// finish[b] = {step at which row b finished or -1, reason}
__global__ void sample_finish_rows_kernel(int64_t* __restrict__ tok, int B, int32_t* __restrict__ state, int32_t* __restrict__ d_pos,
                                          int delta, int n_pos, int64_t* __restrict__ history, int64_t ld_hist, int hist_cols,
                                          int32_t* __restrict__ clear, int n_clear, int clear_stride,
                                          const int32_t* __restrict__ table, int n_eos, int n_seq, int64_t pad,
                                          int32_t* __restrict__ finish) {
  // as in sample_finish_kernel: the step is read once, BEFORE thread 0 bumps it, and broadcast through LDS
  __shared__ int s_step, s_open;
  if (threadIdx.x == 0) { s_step = state[0]; s_open = 0; }
  __syncthreads();
  const int step = s_step;
  for (int i = threadIdx.x; i < n_clear; i += blockDim.x) clear[(int64_t)i * clear_stride] = 0;
  if (d_pos)
    for (int b = threadIdx.x; b < n_pos; b += blockDim.x) d_pos[b] += delta;
  const bool in_hist = history && step >= 0 && step < hist_cols;
  bool open = false;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    int64_t* h = history ? history + (int64_t)b * ld_hist : nullptr;
    int32_t* f = finish + 2 * (int64_t)b;
    if (f[0] >= 0) {                      // finished at an earlier step: padded, never looked at again
      tok[b] = pad;
      if (in_hist) h[step] = pad;
      continue;
    }
    const int64_t t = tok[b];
    if (in_hist) h[step] = t;
    const int code = stop_row_code(t, h, step, step + 1, hist_cols, table, n_eos, n_seq, in_hist);
    if (code) { f[0] = step; f[1] = code; }
    else open = true;
  }
  if (open) atomicOr(&s_open, 1);
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!s_open && state[1] < 0) state[1] = step;
  state[0] = step + 1;
}

// Request streams (DESIGN.md "Request streams"; host statement: sampling.py slot_update): the bookkeeping of a slot session.  The
// launch above with a window per row -- slot[b] = {begin, limit}: the history column of the occupant's first token and its token
// budget --, a RING history (column step % hist_cols, so a session runs for any number of steps) and frozen finished rows: the
// position of a row advances only while it stays open after this step, so an idle slot rewrites one written position and never
// walks past Smax.  The row's own token count is n = (column - begin) mod hist_cols + 1: tokens of the slot's previous occupant
// never take part in a stop sequence, and a row that reaches n >= limit without a match finishes with MG_STOP_LEN.
__global__ void sample_finish_slots_kernel(int64_t* __restrict__ tok, int B, int32_t* __restrict__ state, int32_t* __restrict__ d_pos,
                                           int delta, int64_t* __restrict__ history, int64_t ld_hist, int hist_cols,
                                           int32_t* __restrict__ clear, int n_clear, int clear_stride,
                                           const int32_t* __restrict__ table, int n_eos, int n_seq, int64_t pad,
                                           int32_t* __restrict__ finish, const int32_t* __restrict__ slot) {
  __shared__ int s_step, s_open;
  if (threadIdx.x == 0) { s_step = state[0]; s_open = 0; }
  __syncthreads();
  const int step = s_step;
  for (int i = threadIdx.x; i < n_clear; i += blockDim.x) clear[(int64_t)i * clear_stride] = 0;
  const int col = ((step % hist_cols) + hist_cols) % hist_cols;
  bool open = false;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    int64_t* h = history + (int64_t)b * ld_hist;
    int32_t* f = finish + 2 * (int64_t)b;
    if (f[0] >= 0) {                      // an idle slot: padded, its position stays where it is
      tok[b] = pad;
      h[col] = pad;
      continue;
    }
    const int64_t t = tok[b];
    h[col] = t;
    const int begin = slot[2 * (int64_t)b], limit = slot[2 * (int64_t)b + 1];
    const int n = (((col - begin) % hist_cols) + hist_cols) % hist_cols + 1;
    int code = stop_row_code(t, h, col, n, hist_cols, table, n_eos, n_seq, true);
    if (!code && n >= limit) code = MG_STOP_LEN;
    if (code) { f[0] = step; f[1] = code; }
    else {
      open = true;
      if (d_pos) d_pos[b] += delta;
    }
  }
  if (open) atomicOr(&s_open, 1);
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!s_open && state[1] < 0) state[1] = step;
  state[0] = step + 1;
}

// Speculative greedy decoding (DESIGN.md "Speculative decoding"; host statement: sampling.py speculate_update): the bookkeeping of
// a step that fed T tokens per sequence -- ids[b][0], the last emitted token, and n_draft[b] <= T - 1 guessed continuations -- and
// holds the argmax of every fed row in token[b * token_stride + t].  One workgroup, three phases with a barrier between them:
//   A  thread b, row b: accept the longest prefix of drafts the model agrees with, record the emitted tokens, test them;
//   B  all threads: prompt lookup over the two-segment sequence lookup[b][:len] ++ history[b][:count] of every open row.  For the
//      position c behind a window, m(c) = how many tokens in front of c equal the sequence's last tokens (at most max_ngram, c and
//      L - 1); a window of n tokens in front of c matches iff m(c) >= n, so ONE pass leaves best[b][n] = the first c with m(c) >= n;
//   C  thread b: the largest n with a match gives the drafts; ids and n_draft for the next step; thread 0 latches and counts.
// Device-resident values never form an address unchecked: n_draft counts as clamped into [0, min(T, token_stride) - 1], lookup_len
// into [0, lookup_cols]; a row whose count lies outside [0, history_cols] is skipped whole (nothing of it written, it does not hold
// the loop open); a draft id outside [0, vocab) ends the draft in front of it.
// Stop sequences (mg_spec_finish_seq; n_seq > 0): every emitted token is tested as sample_finish_rows_kernel tests a step's one
// token, so a draft that completes a sequence is accepted, the finishing token is kept and emission is cut behind it.  Drafts are
// still cut only in front of eos ids.  n_seq = 0 is mg_spec_finish.
struct SpecArgs {
  int64_t* ids; int B, T; int32_t* n_draft; const int64_t* token; int token_stride;
  int64_t* history; int64_t ld_hist; int hist_cols; int32_t* count; int32_t* finish;
  const int32_t* table; int n_eos, n_seq, limit; int32_t* d_pos;
  const int32_t* lookup; int64_t ld_lookup; int lookup_cols; const int32_t* lookup_len;
  int32_t* stats; int32_t* state; int num_tokens, max_ngram, vocab;
};
constexpr int SPEC_MAX_ROWS = 16, SPEC_MAX_NGRAM = 16;

__global__ __launch_bounds__(256) void spec_finish_kernel(const SpecArgs a) {
  __shared__ int s_step, s_open;
  __shared__ int s_cnt[SPEC_MAX_ROWS], s_llen[SPEC_MAX_ROWS];                 // an open row's count after this step (-1: no search)
  __shared__ int s_best[SPEC_MAX_ROWS][SPEC_MAX_NGRAM + 1];
  const int tid = threadIdx.x, T = a.T;
  if (tid == 0) { s_step = a.state[0]; s_open = 0; }                         // read once, before thread 0 bumps it
  for (int i = tid; i < SPEC_MAX_ROWS * (SPEC_MAX_NGRAM + 1); i += 256) (&s_best[0][0])[i] = 0x7fffffff;
  if (tid < SPEC_MAX_ROWS) { s_cnt[tid] = -1; s_llen[tid] = 0; }
  __syncthreads();
  const int64_t pad = (int64_t)a.table[0];
  // ---- A: accept, record, test ----
  if (tid < a.B) {
    const int b = tid;
    int64_t* idr = a.ids + (int64_t)b * T;
    int32_t* f = a.finish + 2 * (int64_t)b;
    const int c = a.count[b];
    if (f[0] >= 0) {                                                          // frozen: padded, its position stays
      a.n_draft[b] = 0;
      for (int t = 0; t < T; ++t) idr[t] = pad;
    } else if (c >= 0 && c <= a.hist_cols) {
      int64_t* h = a.history + (int64_t)b * a.ld_hist;
      const int64_t* tk = a.token + (int64_t)b * a.token_stride;
      const int nd = max(0, min(a.n_draft[b], min(T, a.token_stride) - 1));
      int acc = 0;
      while (acc < nd && idr[acc + 1] == tk[acc]) ++acc;
      const int lim = min(a.limit, a.hist_cols);
      int m = 0, code = 0;
      for (int j = 0; j <= acc && c + j < lim && !code; ++j) {
        const int64_t t = tk[j];
        h[c + j] = t;
        m = j + 1;
        // stop_update's rule token by token: eos first, then the stop sequences against the tail of this call's c + j + 1 tokens
        code = stop_row_code(t, h, c + j, c + j + 1, a.hist_cols, a.table, a.n_eos, a.n_seq, a.n_seq > 0);
      }
      if (!code && c + m >= lim) code = MG_STOP_LEN;
      a.count[b] = c + m;
      if (a.d_pos) a.d_pos[b] += m;
      int32_t* st = a.stats + 3 * (int64_t)b;
      st[0] += 1; st[1] += nd; st[2] += acc;
      if (code) {
        f[0] = c + m; f[1] = code;
        a.n_draft[b] = 0;
        for (int t = 0; t < T; ++t) idr[t] = pad;
      } else {
        s_cnt[b] = c + m;
        s_llen[b] = max(0, min(a.lookup_len[b], a.lookup_cols));
      }
    }
  }
  __syncthreads();
  // ---- B: first match of every n-gram size, all open rows ----
  for (int b = 0; b < a.B; ++b) {
    const int cnt = s_cnt[b];
    if (cnt < 0) continue;
    const int llen = s_llen[b], L = llen + cnt, nmax = min(a.max_ngram, L - 1);
    const int32_t* lk = a.lookup + (int64_t)b * a.ld_lookup;
    const int64_t* h = a.history + (int64_t)b * a.ld_hist;
    auto seq = [&](int i) -> int64_t { return i < llen ? (int64_t)lk[i] : h[i - llen]; };
    for (int c = 1 + tid; c < L; c += 256) {
      int m = 0;
      while (m < nmax && m < c && seq(c - 1 - m) == seq(L - 1 - m)) ++m;
      for (int n = 1; n <= m; ++n) atomicMin(&s_best[b][n], c);
    }
  }
  __syncthreads();
  // ---- C: the drafts of the next step ----
  if (tid < a.B && s_cnt[tid] >= 0) {
    const int b = tid, cnt = s_cnt[b], llen = s_llen[b], L = llen + cnt;
    int64_t* idr = a.ids + (int64_t)b * T;
    const int32_t* lk = a.lookup + (int64_t)b * a.ld_lookup;
    const int64_t* h = a.history + (int64_t)b * a.ld_hist;
    auto seq = [&](int i) -> int64_t { return i < llen ? (int64_t)lk[i] : h[i - llen]; };
    const int64_t last = h[cnt - 1];                                           // cnt >= 1: an open row has just emitted a token
    idr[0] = last;
    int nd = 0;
    for (int n = min(a.max_ngram, L - 1); n >= 1; --n) {
      const int c = s_best[b][n];
      if (c == 0x7fffffff) continue;
      const int want = min(min(a.num_tokens, T - 1), L - c);
      for (; nd < want; ++nd) {
        const int64_t t = seq(c + nd);
        bool stop = t < 0 || t >= (int64_t)a.vocab;
        for (int e = 0; e < a.n_eos; ++e) stop = stop || t == (int64_t)a.table[e];
        if (stop) break;
        idr[1 + nd] = t;
      }
      break;                                                                  // the first size with a match decides, as the host rule has it
    }
    for (int t = 1 + nd; t < T; ++t) idr[t] = last;
    a.n_draft[b] = nd;
    atomicOr(&s_open, 1);
  }
  __syncthreads();
  if (tid != 0) return;
  if (!s_open && a.state[1] < 0) a.state[1] = s_step;
  a.state[0] = s_step + 1;
}

// Admission of a slot session: n staged requests installed in one launch.  Block (h, j, l) copies K and V positions
// [pos0, pos0 + len_j) of layer l, head h from staging row src_row[j] to the same positions of live row dst_slot[j] -- len_j * 512
// contiguous bytes each, as 16-byte vectors, all offsets 64-bit --; thread 0 of block (0, j, 0) installs request j's bookkeeping
// and runs the row test on its first token.  pos0 = 0: mg_slots_admit_bf16; pos0 = the session prefix's rows: mg_slots_admit_at_bf16.
// dst0: the live position staged position pos0 goes to -- pos0 for those two; mg_slots_admit_shared_bf16 (a live cache that holds the
// rows' own positions only) passes its own, and d_pos stays the absolute pos0 + len.
struct SlotsAdmitArgs {
  const uint4* kstage; const uint4* vstage; uint4* kcache; uint4* vcache;
  int n_stage, H, S_stage, B, Smax, pos0, dst0;
  int32_t src_row[MG_SLOTS_MAX], dst_slot[MG_SLOTS_MAX], len[MG_SLOTS_MAX], limit[MG_SLOTS_MAX];
  const int64_t* first_token;
  int32_t* state; int32_t* d_pos; int64_t* token; int32_t* finish; int32_t* slot;
  int64_t* history; int64_t ld_hist; int hist_cols;
  const int32_t* table; int n_eos, n_seq;
};

__global__ void slots_admit_kernel(SlotsAdmitArgs a) {
  const int h = blockIdx.x, j = blockIdx.y, l = blockIdx.z;
  const int64_t n_vec = (int64_t)a.len[j] * 32;                 // 256 bf16 = 32 vectors of 16 bytes per position
  const int64_t src = ((((int64_t)l * a.n_stage + a.src_row[j]) * a.H + h) * a.S_stage + a.pos0) * 32;
  const int64_t dst = ((((int64_t)l * a.B + a.dst_slot[j]) * a.H + h) * a.Smax + a.dst0) * 32;
  for (int64_t i = threadIdx.x; i < n_vec; i += blockDim.x) {
    a.kcache[dst + i] = a.kstage[src + i];
    a.vcache[dst + i] = a.vstage[src + i];
  }
  if (threadIdx.x != 0 || h != 0 || l != 0) return;
  const int prev = (int)((unsigned)a.state[0] - 1u);            // the step whose column the first token takes (any value: c below lies in the ring)
  const int c = ((prev % a.hist_cols) + a.hist_cols) % a.hist_cols;
  const int b = a.dst_slot[j];
  const int64_t t = a.first_token[j];
  int64_t* hrow = a.history + (int64_t)b * a.ld_hist;
  a.d_pos[b] = a.pos0 + a.len[j];
  a.token[b] = t;
  a.slot[2 * b] = c;
  a.slot[2 * b + 1] = a.limit[j];
  hrow[c] = t;
  int code = stop_row_code(t, hrow, c, 1, a.hist_cols, a.table, a.n_eos, a.n_seq, true);
  if (!code && a.limit[j] <= 1) code = MG_STOP_LEN;
  a.finish[2 * b] = code ? prev : -1;
  a.finish[2 * b + 1] = code;
  if (j == 0) a.state[1] = -1;
}

}  // namespace

extern "C" int mg_sample_f32(const float* logits, int64_t ld, int32_t B, int32_t V, float temperature, int32_t top_k,
                             double top_p, const uint64_t* seed, const int32_t* state, int64_t* token, float* filtered,
                             int64_t ld_filtered, void* stream) {
  if (B <= 0 || V <= 0 || !logits || ld < V) MG_FAIL(MG_ERR_SHAPE, "mg_sample_f32: bad logits / B / V / ld");
  if (!token && !filtered) MG_FAIL(MG_ERR_SHAPE, "mg_sample_f32: nothing to produce (token and filtered are both null)");
  if (token && (!state || !(temperature > 0.f))) MG_FAIL(MG_ERR_SHAPE, "mg_sample_f32: sampling needs temperature > 0 and a state buffer (greedy decoding is mg_argmax_f32)");
  if (top_k < 0 || top_p < 0.0 || top_p > 1.0) MG_FAIL(MG_ERR_SHAPE, "mg_sample_f32: need top_k >= 0 and 0 <= top_p <= 1");
  if (filtered && ld_filtered < V) MG_FAIL(MG_ERR_SHAPE, "mg_sample_f32: ld_filtered < V");
  SampleParams p{logits, ld, V, temperature, top_k, top_p, seed, state, token, filtered, ld_filtered};
  hipLaunchKernelGGL((sample_kernel<SampleParams, FlatRows>), dim3(B), dim3(ST), 0, (hipStream_t)stream, p, FlatRows{});
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_sample_warp_f32(const float* logits, int64_t ld, int32_t B, int32_t V, float temperature, int32_t top_k,
                                  double top_p, double min_p, const uint64_t* seed, const int32_t* state, int64_t* token,
                                  float* filtered, int64_t ld_filtered, void* stream) {
  if (B <= 0 || V <= 0 || !logits || ld < V) MG_FAIL(MG_ERR_SHAPE, "mg_sample_warp_f32: bad logits / B / V / ld");
  if (!token && !filtered) MG_FAIL(MG_ERR_SHAPE, "mg_sample_warp_f32: nothing to produce (token and filtered are both null)");
  if (!(temperature > 0.f) || temperature == INFINITY) MG_FAIL(MG_ERR_SHAPE, "mg_sample_warp_f32: need a finite temperature > 0 (the filters depend on it)");
  if (token && !state) MG_FAIL(MG_ERR_SHAPE, "mg_sample_warp_f32: sampling needs a state buffer");
  if (top_k < 0 || !(top_p >= 0.0 && top_p <= 1.0) || !(min_p >= 0.0 && min_p <= 1.0))
    MG_FAIL(MG_ERR_SHAPE, "mg_sample_warp_f32: need top_k >= 0, 0 <= top_p <= 1 and 0 <= min_p <= 1");
  if (filtered && ld_filtered < V) MG_FAIL(MG_ERR_SHAPE, "mg_sample_warp_f32: ld_filtered < V");
  WarpParams p{{logits, ld, V, temperature, top_k, top_p, seed, state, token, filtered, ld_filtered},
               min_p > 0.0 ? log(min_p) : -(double)INFINITY};
  hipLaunchKernelGGL((sample_kernel<WarpParams, FlatRows>), dim3(B), dim3(ST), 0, (hipStream_t)stream, p, FlatRows{});
  MG_CHECK_LAUNCH();
  return MG_OK;
}

// Per-request sampling (DESIGN.md "Per-request sampling"): sample_kernel's two instances once more, with TableRows as the source of
// a row's scalars.  The checks cover what the host passes; the table's values are the kernel's to guard (SampleRow above).
extern "C" int mg_sample_rows_f32(const float* logits, int64_t ld, int32_t R, int32_t V, int32_t warp, const void* params,
                                  const int32_t* state, const int32_t* slot, const int32_t* finish, int32_t history_cols,
                                  int64_t* token, float* filtered, int64_t ld_filtered, void* stream) {
  const char* who = "mg_sample_rows_f32";
  if (R <= 0 || V <= 0 || !logits || ld < V) MG_FAIL(MG_ERR_SHAPE, "%s: bad logits / R / V / ld", who);
  if (warp != 0 && warp != 1) MG_FAIL(MG_ERR_SHAPE, "%s: warp must be 0 (the reference's filters) or 1 (transformers' sampler)", who);
  if (!params || !state) MG_FAIL(MG_ERR_SHAPE, "%s: needs the parameter table and a state buffer", who);
  if (!token && !filtered) MG_FAIL(MG_ERR_SHAPE, "%s: nothing to produce (token and filtered are both null)", who);
  if (finish && !slot) MG_FAIL(MG_ERR_SHAPE, "%s: a finish record without the slot table (the static call skips no row)", who);
  if (slot && !finish) MG_FAIL(MG_ERR_SHAPE, "%s: the slot table without the finish record", who);
  if (slot && history_cols <= 0) MG_FAIL(MG_ERR_SHAPE, "%s: a slot session's ring has history_cols > 0", who);
  if (filtered && ld_filtered < V) MG_FAIL(MG_ERR_SHAPE, "%s: ld_filtered < V", who);
  if (!MG_ALIGNED16(params)) MG_FAIL(MG_ERR_ALIGN, "%s: the parameter table must be 16-byte aligned", who);
  if (((uintptr_t)logits | (uintptr_t)state | (uintptr_t)slot | (uintptr_t)finish | (uintptr_t)filtered) & 3)
    MG_FAIL(MG_ERR_ALIGN, "%s: fp32 / int32 buffers must be 4-byte aligned", who);
  if ((uintptr_t)token & 7) MG_FAIL(MG_ERR_ALIGN, "%s: the token buffer must be 8-byte aligned", who);
  const TableRows src{(const SampleRow*)params, slot, finish, history_cols};
  const SampleParams p{logits, ld, V, 1.0f, 0, 0.0, nullptr, state, token, filtered, ld_filtered};
  if (warp) {
    const WarpParams w{p, -(double)INFINITY};
    hipLaunchKernelGGL((sample_kernel<WarpParams, TableRows>), dim3(R), dim3(ST), 0, (hipStream_t)stream, w, src);
  } else {
    hipLaunchKernelGGL((sample_kernel<SampleParams, TableRows>), dim3(R), dim3(ST), 0, (hipStream_t)stream, p, src);
  }
  MG_CHECK_LAUNCH();
  return MG_OK;
}

// The selection launch of a speculative step (DESIGN.md "Speculative decoding"): sample_kernel's two instances a third time, with
// ChunkRows as the source -- one workgroup per fed row b * T + t, sequence b's record, the draw at counter count[b] + t.  The checks
// are mg_sample_rows_f32's; the records, count and n_draft are device values the kernel clamps or skips on.
extern "C" int mg_sample_chunk_f32(const float* logits, int64_t ld, int32_t B, int32_t T, int32_t V, int32_t warp, const void* params,
                                   const int32_t* count, const int32_t* n_draft, const int32_t* finish, int32_t history_cols,
                                   int64_t* token, float* filtered, int64_t ld_filtered, void* stream) {
  const char* who = "mg_sample_chunk_f32";
  if (B <= 0 || V <= 0 || !logits || ld < V) MG_FAIL(MG_ERR_SHAPE, "%s: bad logits / B / V / ld", who);
  if (T < 1 || T > 8 || (int64_t)B * T > 16) MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= T <= 8 and B * T <= 16, got B = %d, T = %d", who, B, T);
  if (warp != 0 && warp != 1) MG_FAIL(MG_ERR_SHAPE, "%s: warp must be 0 (the reference's filters) or 1 (transformers' sampler)", who);
  if (!params || !count || !finish) MG_FAIL(MG_ERR_SHAPE, "%s: needs the parameter table, count and the finish record", who);
  if (!token && !filtered) MG_FAIL(MG_ERR_SHAPE, "%s: nothing to produce (token and filtered are both null)", who);
  if (history_cols < 0) MG_FAIL(MG_ERR_SHAPE, "%s: history_cols < 0", who);
  if (filtered && ld_filtered < V) MG_FAIL(MG_ERR_SHAPE, "%s: ld_filtered < V", who);
  if (!MG_ALIGNED16(params)) MG_FAIL(MG_ERR_ALIGN, "%s: the parameter table must be 16-byte aligned", who);
  if (((uintptr_t)logits | (uintptr_t)count | (uintptr_t)n_draft | (uintptr_t)finish | (uintptr_t)filtered) & 3)
    MG_FAIL(MG_ERR_ALIGN, "%s: fp32 / int32 buffers must be 4-byte aligned", who);
  if ((uintptr_t)token & 7) MG_FAIL(MG_ERR_ALIGN, "%s: the token buffer must be 8-byte aligned", who);
  const ChunkRows src{(const SampleRow*)params, count, n_draft, finish, history_cols, T};
  const SampleParams p{logits, ld, V, 1.0f, 0, 0.0, nullptr, nullptr, token, filtered, ld_filtered};
  if (warp) {
    const WarpParams w{p, -(double)INFINITY};
    hipLaunchKernelGGL((sample_kernel<WarpParams, ChunkRows>), dim3(B * T), dim3(ST), 0, (hipStream_t)stream, w, src);
  } else {
    hipLaunchKernelGGL((sample_kernel<SampleParams, ChunkRows>), dim3(B * T), dim3(ST), 0, (hipStream_t)stream, p, src);
  }
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_sample_finish(const int64_t* token, int32_t B, int64_t eos, int32_t* state, int32_t* d_pos, int32_t delta,
                                int64_t* history, int64_t ld_history, int32_t history_cols, int32_t* clear, int32_t n_clear,
                                int32_t clear_stride, int32_t pos_stride, void* stream) {
  if (!token || !state || B <= 0) MG_FAIL(MG_ERR_SHAPE, "mg_sample_finish: bad arguments");
  if (pos_stride != 0 && pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "mg_sample_finish: pos_stride must be 0 or 1");
  if (history && (ld_history < history_cols || history_cols <= 0)) MG_FAIL(MG_ERR_SHAPE, "mg_sample_finish: bad history geometry");
  hipLaunchKernelGGL(sample_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, token, B, eos, state, d_pos, delta,
                     pos_stride ? B : 1,
                     history, ld_history, history_cols, clear, clear ? n_clear : 0, clear_stride > 0 ? clear_stride : 1);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_sample_finish_rows(int64_t* token, int32_t B, int32_t* state, int32_t* d_pos, int32_t delta, int64_t* history,
                                     int64_t ld_history, int32_t history_cols, int32_t* clear, int32_t n_clear, int32_t clear_stride,
                                     int32_t pos_stride, const int32_t* table, int32_t n_eos, int32_t n_seq, int64_t pad,
                                     int32_t* finish, void* stream) {
  if (!token || !state || !table || !finish || B <= 0) MG_FAIL(MG_ERR_SHAPE, "mg_sample_finish_rows: bad arguments");
  if (pos_stride != 0 && pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "mg_sample_finish_rows: pos_stride must be 0 or 1");
  if (history && (ld_history < history_cols || history_cols <= 0)) MG_FAIL(MG_ERR_SHAPE, "mg_sample_finish_rows: bad history geometry");
  if (n_eos < 1 || n_eos > MG_STOP_MAX_EOS || n_seq < 0 || n_seq > MG_STOP_MAX_SEQ)
    MG_FAIL(MG_ERR_SHAPE, "mg_sample_finish_rows: need 1 <= n_eos <= %d and 0 <= n_seq <= %d, got %d / %d", MG_STOP_MAX_EOS,
            MG_STOP_MAX_SEQ, n_eos, n_seq);
  if (n_seq > 0 && !history) MG_FAIL(MG_ERR_SHAPE, "mg_sample_finish_rows: stop sequences are matched against the token history: it is missing");
  hipLaunchKernelGGL(sample_finish_rows_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, token, B, state, d_pos, delta,
                     pos_stride ? B : 1, history, ld_history, history ? history_cols : 0, clear, clear ? n_clear : 0,
                     clear_stride > 0 ? clear_stride : 1, table, n_eos, n_seq, pad, finish);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_sample_finish_slots(int64_t* token, int32_t B, int32_t* state, int32_t* d_pos, int32_t delta, int64_t* history,
                                      int64_t ld_history, int32_t history_cols, int32_t* clear, int32_t n_clear, int32_t clear_stride,
                                      int32_t pos_stride, const int32_t* table, int32_t n_eos, int32_t n_seq, int64_t pad,
                                      int32_t* finish, const int32_t* slot, void* stream) {
  const char* who = "mg_sample_finish_slots";
  if (!token || !state || !table || !finish || !slot || B <= 0) MG_FAIL(MG_ERR_SHAPE, "%s: bad arguments", who);
  if (d_pos && pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "%s: a slot session keeps one position per row (pos_stride must be 1)", who);
  if (!history || history_cols <= 0 || ld_history < history_cols) MG_FAIL(MG_ERR_SHAPE, "%s: needs a ring history with 0 < history_cols <= ld_history", who);
  if (n_eos < 1 || n_eos > MG_STOP_MAX_EOS || n_seq < 0 || n_seq > MG_STOP_MAX_SEQ)
    MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= n_eos <= %d and 0 <= n_seq <= %d, got %d / %d", who, MG_STOP_MAX_EOS, MG_STOP_MAX_SEQ, n_eos, n_seq);
  hipLaunchKernelGGL(sample_finish_slots_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, token, B, state, d_pos, delta, history,
                     ld_history, history_cols, clear, clear ? n_clear : 0, clear_stride > 0 ? clear_stride : 1, table, n_eos, n_seq, pad,
                     finish, slot);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

static int spec_finish_launch(const char* who, int64_t* ids, int32_t B, int32_t T, int32_t* n_draft, const int64_t* token,
                              int32_t token_stride, int64_t* history, int64_t ld_history, int32_t history_cols, int32_t* count,
                              int32_t* finish, const int32_t* table, int32_t n_eos, int32_t n_seq, int32_t limit, int32_t* d_pos,
                              const int32_t* lookup, int64_t ld_lookup, int32_t lookup_cols, const int32_t* lookup_len,
                              int32_t* stats, int32_t* state, int32_t num_tokens, int32_t max_ngram, int32_t vocab, void* stream) {
  if (!ids || !n_draft || !token || !history || !count || !finish || !table || !lookup_len || !stats || !state || (lookup_cols > 0 && !lookup))
    MG_FAIL(MG_ERR_SHAPE, "%s: null pointer", who);
  if (B < 1 || B > SPEC_MAX_ROWS || T < 2 || T > 8 || B * T > 16) MG_FAIL(MG_ERR_SHAPE, "%s: need 2 <= T <= 8 and B * T <= 16, got B = %d, T = %d", who, B, T);
  if (token_stride != 1 && token_stride != T) MG_FAIL(MG_ERR_SHAPE, "%s: token_stride is T (a step's rows) or 1 (the arming call), got %d", who, token_stride);
  if (history_cols <= 0 || ld_history < history_cols) MG_FAIL(MG_ERR_SHAPE, "%s: bad history geometry", who);
  if (lookup_cols < 0 || ld_lookup < lookup_cols) MG_FAIL(MG_ERR_SHAPE, "%s: bad lookup geometry", who);
  if ((int64_t)lookup_cols + history_cols > 0x7fffff00) MG_FAIL(MG_ERR_SHAPE, "%s: lookup_cols + history_cols must stay below 2^31", who);
  if (n_eos < 1 || n_eos > MG_STOP_MAX_EOS) MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= n_eos <= %d, got %d", who, MG_STOP_MAX_EOS, n_eos);
  if (n_seq < 0 || n_seq > MG_STOP_MAX_SEQ) MG_FAIL(MG_ERR_SHAPE, "%s: need 0 <= n_seq <= %d, got %d", who, MG_STOP_MAX_SEQ, n_seq);
  if (num_tokens < 1 || num_tokens > T - 1 || max_ngram < 1 || max_ngram > SPEC_MAX_NGRAM)
    MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= num_tokens <= T - 1 and 1 <= max_ngram <= %d, got %d / %d", who, SPEC_MAX_NGRAM, num_tokens, max_ngram);
  if (limit < 0 || vocab < 1) MG_FAIL(MG_ERR_SHAPE, "%s: need limit >= 0 and vocab >= 1", who);
  if (((uintptr_t)n_draft | (uintptr_t)count | (uintptr_t)finish | (uintptr_t)table | (uintptr_t)d_pos | (uintptr_t)lookup |
       (uintptr_t)lookup_len | (uintptr_t)stats | (uintptr_t)state) & 3)
    MG_FAIL(MG_ERR_ALIGN, "%s: int32 buffers must be 4-byte aligned", who);
  if (((uintptr_t)ids | (uintptr_t)token | (uintptr_t)history) & 7) MG_FAIL(MG_ERR_ALIGN, "%s: token buffers must be 8-byte aligned", who);
  const SpecArgs a{ids, B, T, n_draft, token, token_stride, history, ld_history, history_cols, count, finish, table, n_eos, n_seq, limit,
                   d_pos, lookup, ld_lookup, lookup_cols, lookup_len, stats, state, num_tokens, max_ngram, vocab};
  hipLaunchKernelGGL(spec_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_spec_finish(int64_t* ids, int32_t B, int32_t T, int32_t* n_draft, const int64_t* token, int32_t token_stride,
                              int64_t* history, int64_t ld_history, int32_t history_cols, int32_t* count, int32_t* finish,
                              const int32_t* table, int32_t n_eos, int32_t limit, int32_t* d_pos, const int32_t* lookup,
                              int64_t ld_lookup, int32_t lookup_cols, const int32_t* lookup_len, int32_t* stats, int32_t* state,
                              int32_t num_tokens, int32_t max_ngram, int32_t vocab, void* stream) {
  return spec_finish_launch("mg_spec_finish", ids, B, T, n_draft, token, token_stride, history, ld_history, history_cols, count, finish,
                            table, n_eos, 0, limit, d_pos, lookup, ld_lookup, lookup_cols, lookup_len, stats, state, num_tokens,
                            max_ngram, vocab, stream);
}

// mg_spec_finish with stop sequences: `table` is the full MG_STOP_TABLE_INTS table of mg_sample_finish_rows, n_seq of its sequences live.
extern "C" int mg_spec_finish_seq(int64_t* ids, int32_t B, int32_t T, int32_t* n_draft, const int64_t* token, int32_t token_stride,
                                  int64_t* history, int64_t ld_history, int32_t history_cols, int32_t* count, int32_t* finish,
                                  const int32_t* table, int32_t n_eos, int32_t n_seq, int32_t limit, int32_t* d_pos,
                                  const int32_t* lookup, int64_t ld_lookup, int32_t lookup_cols, const int32_t* lookup_len,
                                  int32_t* stats, int32_t* state, int32_t num_tokens, int32_t max_ngram, int32_t vocab, void* stream) {
  return spec_finish_launch("mg_spec_finish_seq", ids, B, T, n_draft, token, token_stride, history, ld_history, history_cols, count,
                            finish, table, n_eos, n_seq, limit, d_pos, lookup, ld_lookup, lookup_cols, lookup_len, stats, state,
                            num_tokens, max_ngram, vocab, stream);
}

// The admission entry points: the checks and the one launch.
static int slots_admit_launch(const char* who, const mg_bf16* kstage, const mg_bf16* vstage, int32_t n_stage, int32_t S_stage,
                              mg_bf16* kcache, mg_bf16* vcache, int32_t L, int32_t B, int32_t H, int32_t Smax, int32_t n,
                              const int32_t* src_row, const int32_t* dst_slot, const int32_t* len, const int64_t* first_token,
                              const int32_t* limit, int32_t* state, int32_t* d_pos, int64_t* token, int32_t* finish, int32_t* slot,
                              int64_t* history, int64_t ld_history, int32_t history_cols, const int32_t* table, int32_t n_eos,
                              int32_t n_seq, int32_t pos0, int32_t dst0, void* stream) {
  if (!kstage || !vstage || !kcache || !vcache || !src_row || !dst_slot || !len || !first_token || !limit || !state || !d_pos || !token ||
      !finish || !slot || !history || !table)
    MG_FAIL(MG_ERR_SHAPE, "%s: null pointer", who);
  if (L <= 0 || B <= 0 || H <= 0 || Smax <= 0 || n_stage <= 0 || S_stage <= 0) MG_FAIL(MG_ERR_SHAPE, "%s: bad cache geometry", who);
  if (H > 65535 || L > 65535) MG_FAIL(MG_ERR_SHAPE, "%s: grid too large", who);
  if (n < 1 || n > B || n > MG_SLOTS_MAX) MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= n <= min(B, %d), got n = %d at B = %d", who, MG_SLOTS_MAX, n, B);
  if (history_cols <= 0 || ld_history < history_cols) MG_FAIL(MG_ERR_SHAPE, "%s: bad history geometry", who);
  if (n_eos < 1 || n_eos > MG_STOP_MAX_EOS || n_seq < 0 || n_seq > MG_STOP_MAX_SEQ)
    MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= n_eos <= %d and 0 <= n_seq <= %d, got %d / %d", who, MG_STOP_MAX_EOS, MG_STOP_MAX_SEQ, n_eos, n_seq);
  if (!MG_ALIGNED16(kstage) || !MG_ALIGNED16(vstage) || !MG_ALIGNED16(kcache) || !MG_ALIGNED16(vcache))
    MG_FAIL(MG_ERR_ALIGN, "%s: the caches must be 16-byte aligned", who);
  if (((uintptr_t)state | (uintptr_t)d_pos | (uintptr_t)finish | (uintptr_t)slot | (uintptr_t)table) & 3)
    MG_FAIL(MG_ERR_ALIGN, "%s: int32 buffers must be 4-byte aligned", who);
  if (((uintptr_t)token | (uintptr_t)history | (uintptr_t)first_token) & 7) MG_FAIL(MG_ERR_ALIGN, "%s: token buffers must be 8-byte aligned", who);
  SlotsAdmitArgs a{};
  // each side against its own extent (equal offsets: pos0 inside [0, min(S_stage, Smax)), as ever)
  if (pos0 < 0 || pos0 >= S_stage) MG_FAIL(MG_ERR_SHAPE, "%s: pos0 = %d outside [0, %d)", who, pos0, S_stage);
  if (dst0 < 0 || dst0 >= Smax) MG_FAIL(MG_ERR_SHAPE, "%s: %s = %d outside [0, %d)", who, dst0 == pos0 ? "pos0" : "dst0", dst0, Smax);
  const int len_max = S_stage - pos0 < Smax - dst0 ? S_stage - pos0 : Smax - dst0;
  for (int j = 0; j < n; ++j) {
    if (src_row[j] < 0 || src_row[j] >= n_stage) MG_FAIL(MG_ERR_SHAPE, "%s: src_row[%d] = %d outside [0, %d)", who, j, src_row[j], n_stage);
    if (dst_slot[j] < 0 || dst_slot[j] >= B) MG_FAIL(MG_ERR_SHAPE, "%s: dst_slot[%d] = %d outside [0, %d)", who, j, dst_slot[j], B);
    for (int i = 0; i < j; ++i)
      if (dst_slot[i] == dst_slot[j]) MG_FAIL(MG_ERR_SHAPE, "%s: slot %d is the target of requests %d and %d", who, dst_slot[j], i, j);
    if (len[j] < 1 || len[j] > len_max) MG_FAIL(MG_ERR_SHAPE, "%s: len[%d] = %d outside [1, %d]", who, j, len[j], len_max);
    a.src_row[j] = src_row[j]; a.dst_slot[j] = dst_slot[j]; a.len[j] = len[j]; a.limit[j] = limit[j];
  }
  a.kstage = (const uint4*)kstage; a.vstage = (const uint4*)vstage; a.kcache = (uint4*)kcache; a.vcache = (uint4*)vcache;
  a.n_stage = n_stage; a.H = H; a.S_stage = S_stage; a.B = B; a.Smax = Smax; a.pos0 = pos0; a.dst0 = dst0;
  a.first_token = first_token; a.state = state; a.d_pos = d_pos; a.token = token; a.finish = finish; a.slot = slot;
  a.history = history; a.ld_hist = ld_history; a.hist_cols = history_cols; a.table = table; a.n_eos = n_eos; a.n_seq = n_seq;
  hipLaunchKernelGGL(slots_admit_kernel, dim3(H, n, L), dim3(256), 0, (hipStream_t)stream, a);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_slots_admit_bf16(const mg_bf16* kstage, const mg_bf16* vstage, int32_t n_stage, int32_t S_stage, mg_bf16* kcache,
                                   mg_bf16* vcache, int32_t L, int32_t B, int32_t H, int32_t Smax, int32_t n, const int32_t* src_row,
                                   const int32_t* dst_slot, const int32_t* len, const int64_t* first_token, const int32_t* limit,
                                   int32_t* state, int32_t* d_pos, int64_t* token, int32_t* finish, int32_t* slot, int64_t* history,
                                   int64_t ld_history, int32_t history_cols, const int32_t* table, int32_t n_eos, int32_t n_seq,
                                   void* stream) {
  return slots_admit_launch("mg_slots_admit_bf16", kstage, vstage, n_stage, S_stage, kcache, vcache, L, B, H, Smax, n, src_row, dst_slot,
                            len, first_token, limit, state, d_pos, token, finish, slot, history, ld_history, history_cols, table, n_eos,
                            n_seq, 0, 0, stream);
}

extern "C" int mg_slots_admit_at_bf16(const mg_bf16* kstage, const mg_bf16* vstage, int32_t n_stage, int32_t S_stage, mg_bf16* kcache,
                                      mg_bf16* vcache, int32_t L, int32_t B, int32_t H, int32_t Smax, int32_t n, const int32_t* src_row,
                                      const int32_t* dst_slot, const int32_t* len, const int64_t* first_token, const int32_t* limit,
                                      int32_t* state, int32_t* d_pos, int64_t* token, int32_t* finish, int32_t* slot, int64_t* history,
                                      int64_t ld_history, int32_t history_cols, const int32_t* table, int32_t n_eos, int32_t n_seq,
                                      int32_t pos0, void* stream) {
  return slots_admit_launch("mg_slots_admit_at_bf16", kstage, vstage, n_stage, S_stage, kcache, vcache, L, B, H, Smax, n, src_row,
                            dst_slot, len, first_token, limit, state, d_pos, token, finish, slot, history, ld_history, history_cols,
                            table, n_eos, n_seq, pos0, pos0, stream);
}

extern "C" int mg_slots_admit_shared_bf16(const mg_bf16* kstage, const mg_bf16* vstage, int32_t n_stage, int32_t S_stage, mg_bf16* kcache,
                                          mg_bf16* vcache, int32_t L, int32_t B, int32_t H, int32_t Smax, int32_t n,
                                          const int32_t* src_row, const int32_t* dst_slot, const int32_t* len,
                                          const int64_t* first_token, const int32_t* limit, int32_t* state, int32_t* d_pos,
                                          int64_t* token, int32_t* finish, int32_t* slot, int64_t* history, int64_t ld_history,
                                          int32_t history_cols, const int32_t* table, int32_t n_eos, int32_t n_seq, int32_t pos0,
                                          int32_t dst0, void* stream) {
  return slots_admit_launch("mg_slots_admit_shared_bf16", kstage, vstage, n_stage, S_stage, kcache, vcache, L, B, H, Smax, n, src_row,
                            dst_slot, len, first_token, limit, state, d_pos, token, finish, slot, history, ld_history, history_cols,
                            table, n_eos, n_seq, pos0, dst0, stream);
}

// ================================================================================================================================
// Beam search (DESIGN.md "Beam search"): the rule of transformers' vectorised GenerationMixin._beam_search with do_sample=False
// and one eos id, restated on the host in magma_amd/sampling.py (beam_search), as three enqueue-only launches per token step:
//   beam_topk_kernel    one workgroup per row (B*k rows): max and logsumexp of the row, then the top 2k of that row's candidate
//                       scores  run[row] + ((x - max) - lse)  in the order (score descending, lower token first) -- the radix
//                       descent of sample_kernel's top-k on the order-preserving keys of the SCORES (so that equal fp32 scores
//                       are ordered by index exactly as the per-sample merge orders them), ties at the threshold cut by index
//                       with one wave and ballots.  A sample's top 2k over k*V candidates lie in the union of its rows' top 2k.
//   beam_finish_kernel  one workgroup: per sample, the merge of the k lists by (score desc, flat index beam*V + token asc), the
//                       finish / next-beam / early-stop rules, the parent map, the token histories gathered by parent, the
//                       finished hypotheses, the fed-back token, d_pos and the "first step at which generation stops" record.
//                       beam_finish_groups_kernel (DESIGN.md "Diverse beam search") is the same body walking the G groups of
//                       every sample as samples of k / G beams, a group's candidates penalised for the tokens that the
//                       sample's earlier groups selected at this step; its rows' lists are k + k / G long.
//   kv_reorder_kernel   K / V positions [0, d_pos_b) of row parent[b] into row b, every layer, in two launches: rows that are
//                       read by another row AND are themselves overwritten are staged first; identity rows are skipped.
namespace {

constexpr int BK_MAX = 16;              // largest num_beams
constexpr int BK2_MAX = 2 * BK_MAX;

// The max / logsumexp of a vocabulary row and, from them, the top K2 entries of the row -- ONE body for the beam step's candidate
// lists and for the token log-probabilities (mg_token_logprobs_f32), so that both form (x - max) - lse with the same arithmetic
// and the same reduction tree.  x = the row, out_score / out_tok = the row's K2 output slots.
// PRE: the row already holds log_softmax (and the logits processors' -inf) -- logits_process_kernel with normalize = 1 wrote
// (x - max) - lse with the arithmetic below -- so a candidate's score is run + x.
// RAW: the entries are ranked by the raw logit (descending, lower token first) instead of by the score, and the value written is
// (x - max) - lse itself (no running score): the order is then a function of the logits alone.  K2 = 0: no selection pass.
// Compile-time branches of one body: the instances without RAW are the beam kernels as they were.
struct RowLse { float mx, lse; };

template <bool PRE, bool RAW>
MG_DEV RowLse row_topk_body(const float* __restrict__ x, int V, float r, int K2, float* __restrict__ out_score,
                            int32_t* __restrict__ out_tok) {
  __shared__ uint32_t hist32[256];
  __shared__ float shf[ST / 64];
  __shared__ uint32_t bc[4];
  __shared__ int s_cut, s_n;
  __shared__ uint32_t s_key[BK2_MAX];
  __shared__ int s_idx[BK2_MAX];
  __shared__ float s_sc[BK2_MAX];
  const int tid = threadIdx.x;

  float mx = -INFINITY, lse = 0.f;
  if constexpr (!PRE) {
    for (int i = tid; i < V; i += ST) mx = fmaxf(mx, x[i]);
    mx = blk_max(mx, shf);
    float z = 0.f;
    for (int i = tid; i < V; i += ST) z += expf(x[i] - mx);
    z = blk_sum(z, shf);
    lse = logf(z);
  }
  const RowLse stat{mx, lse};
  if (K2 <= 0) return stat;                // (uniform over the workgroup)
  auto score = [&](int i) -> float {       // log_softmax, then the running score
    if constexpr (PRE) return r + x[i];
    else if constexpr (RAW) return (x[i] - mx) - lse;
    else return r + ((x[i] - mx) - lse);
  };
  auto key = [&](int i) -> uint32_t {      // what the entries are ranked by
    if constexpr (RAW) return fkey(x[i]);
    else return fkey(score(i));
  };

  // key of the K2-th largest score (MSB-first radix descent, 8 bits per level)
  uint32_t prefix = 0, mask = 0, remaining = (uint32_t)K2, in_bucket = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist32[tid] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += ST) {
      const uint32_t k = key(i);
      if ((k & mask) == prefix) atomicAdd(&hist32[(k >> shift) & 255], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t rem = remaining; int d = 0;
      for (int b = 255; b >= 0; --b) {
        if (hist32[b] >= rem) { d = b; break; }
        rem -= hist32[b];
      }
      bc[0] = (uint32_t)d; bc[1] = rem; bc[2] = hist32[d];
    }
    __syncthreads();
    prefix |= bc[0] << shift; mask |= 255u << shift; remaining = bc[1]; in_bucket = bc[2];
    __syncthreads();
  }
  const uint32_t tk = prefix;
  // the candidates: every key above tk, and the first `remaining` keys equal to it by index (cut = index of the first tie left out)
  if (tid == 0) { s_cut = 0x7fffffff; s_n = 0; }
  __syncthreads();
  if (in_bucket > remaining && tid < 64) {
    uint32_t seen = 0;
    for (int base = 0; base < V; base += 64) {
      const int i = base + tid;
      const bool eq = i < V && key(i) == tk;
      const unsigned long long m = __ballot(eq);
      const uint32_t c = (uint32_t)__popcll(m);
      if (seen + c > remaining) {
        if (eq && (uint32_t)__popcll(m & ((1ull << tid) - 1ull)) == remaining - seen) s_cut = i;
        break;
      }
      seen += c;
    }
  }
  __syncthreads();
  const int cut = s_cut;
  for (int i = tid; i < V; i += ST) {
    const uint32_t k = key(i);
    if (k > tk || (k == tk && i < cut)) {
      const int slot = atomicAdd(&s_n, 1);
      if (slot < BK2_MAX) { s_key[slot] = k; s_idx[slot] = i; s_sc[slot] = score(i); }
    }
  }
  __syncthreads();
  const int n = min(s_n, K2);
  if (tid < n) {      // rank by (key desc, index asc): a fixed order whatever order the atomics handed out the slots in
    const uint32_t k = s_key[tid]; const int i = s_idx[tid];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (s_key[j] > k || (s_key[j] == k && s_idx[j] < i)) ? 1 : 0;
    out_score[rank] = s_sc[tid];
    out_tok[rank] = i;
  }
  return stat;
}

template <bool PRE>
MG_DEV void beam_topk_body(const float* __restrict__ logits, int64_t ld, int V, const float* __restrict__ run, int K2,
                           float* __restrict__ cand_score, int32_t* __restrict__ cand_tok) {
  const int row = blockIdx.x;
  row_topk_body<PRE, false>(logits + (int64_t)row * ld, V, run[row], K2, cand_score + (int64_t)row * K2, cand_tok + (int64_t)row * K2);
}

__global__ __launch_bounds__(ST) void beam_topk_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                       const float* __restrict__ run, int K2, float* __restrict__ cand_score,
                                                       int32_t* __restrict__ cand_tok) {
  beam_topk_body<false>(logits, ld, V, run, K2, cand_score, cand_tok);
}
__global__ __launch_bounds__(ST) void beam_topk_pre_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                           const float* __restrict__ run, int K2, float* __restrict__ cand_score,
                                                           int32_t* __restrict__ cand_tok) {
  beam_topk_body<true>(logits, ld, V, run, K2, cand_score, cand_tok);
}

// Token log-probabilities (DESIGN.md "Token log-probabilities"; host statement: sampling.py token_logprobs): per row the
// log-probability of the row's token and the n_top most probable tokens, from row_topk_body's max / logsumexp -- the arithmetic
// of the beam step -- ranked by the raw logit.  One workgroup per row; column c = state[0] of the per-step buffers (0 without a
// state); c outside [0, cols) writes nothing; a token outside [0, V) reads nothing and gives -inf.
MG_DEV void token_logprobs_body(const float* __restrict__ logits, int64_t ld, int V, const int64_t* __restrict__ token, int c,
                                float* __restrict__ lp, int64_t ld_lp, int cols, int n_top, int32_t* __restrict__ top_id,
                                float* __restrict__ top_lp) {
  const int row = blockIdx.x;
  if (c < 0 || c >= cols) return;            // (uniform over the workgroup)
  const float* x = logits + (int64_t)row * ld;
  const int64_t slot = ((int64_t)row * cols + c) * n_top;
  const RowLse s = row_topk_body<false, true>(x, V, 0.f, n_top, top_lp + slot, top_id + slot);
  if (threadIdx.x == 0) {
    const int64_t t = token[row];
    lp[(int64_t)row * ld_lp + c] = t >= 0 && t < V ? (x[t] - s.mx) - s.lse : -INFINITY;
  }
}

__global__ __launch_bounds__(ST) void token_logprobs_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                            const int64_t* __restrict__ token, const int32_t* __restrict__ state,
                                                            float* __restrict__ lp, int64_t ld_lp, int cols, int n_top,
                                                            int32_t* __restrict__ top_id, float* __restrict__ top_lp) {
  token_logprobs_body(logits, ld, V, token, state ? state[0] : 0, lp, ld_lp, cols, n_top, top_id, top_lp);
}

// A row's tokens so far, as the logits processors and the trie walk read them (DESIGN.md "Choosing over a request stream"): token
// i = 0 .. len - 1 at h[(begin + i) % cols].  RING = false is the plain history -- begin = 0, len <= cols, h[i] as it always was --;
// RING = true is a slot's window of the ring history, walked across the wrap (begin in [0, cols), len in [1, cols]: one
// conditional subtraction, in unsigned arithmetic, is the modulus).
template <bool RING>
struct HistView {
  const int64_t* h; int begin, len, cols;
  MG_DEV int64_t operator[](int i) const {
    if constexpr (!RING) return h[i];
    else {
      uint32_t c = (uint32_t)begin + (uint32_t)i;
      if (c >= (uint32_t)cols) c -= (uint32_t)cols;
      return h[c];
    }
  }
};

// mg_token_logprobs_slots_f32: the body above at column n of an occupied row (column 0 is the admission's); an idle row and a
// column at or beyond cols write nothing.
__global__ __launch_bounds__(ST) void token_logprobs_slots_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                                  const int64_t* __restrict__ token, const int32_t* __restrict__ state,
                                                                  float* __restrict__ lp, int64_t ld_lp, int cols, int n_top,
                                                                  int32_t* __restrict__ top_id, float* __restrict__ top_lp,
                                                                  const int32_t* __restrict__ slot, const int32_t* __restrict__ finish,
                                                                  int hist_cols) {
  const SlotWin w = slot_window(state, slot, finish, blockIdx.x, hist_cols);
  if (w.n == 0) return;                      // (uniform over the workgroup)
  token_logprobs_body(logits, ld, V, token, w.n, lp, ld_lp, cols, n_top, top_id, top_lp);
}

// Classifier-free guidance (DESIGN.md "Classifier-free guidance"; host statement: sampling.py guide_logits): the rule of transformers'
// UnbatchedClassifierFreeGuidanceLogitsProcessor -- out = u + scale * (c - u) over the log_softmax c of the conditional row and u of
// the unconditional one -- and the plausibility cut of contrastive decoding on the RAW conditional logits, in place on the
// conditional row.  One workgroup per pair of rows.  row_topk_body's max / logsumexp takes two sweeps per row; over a pair that
// would be four sweeps and the output pass a fifth, so the two sweeps are folded into ONE: every thread keeps a running (maximum,
// sum of exp(x - maximum)) per row, rescaling its sum when its maximum grows; the workgroup's maximum comes from blk_max, every
// thread's sum is rescaled to it once and added by blk_sum -- the same fixed trees.  The output is formed by row_topk_body's
// expression (x - max) - lse.  Which thread adds which elements, and in which order, depends on the element INDEX alone -- groups of
// four from index 0, the last V % 4 elements one per thread -- never on where the row lies: equal rows give equal bits (and c - u = 0
// exactly) wherever they sit, and a row gives the same values in the prefill's buffer as in the step's.  A row start is only 4-byte
// aligned in general; a group is loaded (and stored) as one 16-byte access where the row allows it, as two 8-byte ones where it
// allows those, else as four dwords -- the step's own logits rows (ld a multiple of 8) take the first form.
MG_DEV void online_acc(float v, float& m, float& z) {
  if (v > m) { z *= expf(m - v); m = v; }             // (m = -inf: z is 0 and stays 0)
  if (v > -INFINITY) z += expf(v - m);
}
MG_DEV void online_acc4(const float4 q, float& m, float& z) {
  const float vm = fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w));
  if (vm > m) { z *= expf(m - vm); m = vm; }
  if (vm > -INFINITY) z += (expf(q.x - m) + expf(q.y - m)) + (expf(q.z - m) + expf(q.w - m));
}
MG_DEV int row_align(const float* x) {                // 2: 16-byte aligned, 1: 8-byte, 0: 4-byte (the same for every group of the row)
  const uint32_t a = (uint32_t)(uintptr_t)x & 15u;
  return a == 0u ? 2 : a == 8u ? 1 : 0;
}
MG_DEV float4 load4(const float* p, int al) {
  if (al == 2) return *reinterpret_cast<const float4*>(p);
  if (al == 1) {
    const float2 a = *reinterpret_cast<const float2*>(p), b = *reinterpret_cast<const float2*>(p + 2);
    return make_float4(a.x, a.y, b.x, b.y);
  }
  return make_float4(p[0], p[1], p[2], p[3]);
}
MG_DEV void store4(float* p, int al, const float4 v) {
  if (al == 2) *reinterpret_cast<float4*>(p) = v;
  else if (al == 1) { *reinterpret_cast<float2*>(p) = make_float2(v.x, v.y); *reinterpret_cast<float2*>(p + 2) = make_float2(v.z, v.w); }
  else { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
}
MG_DEV void row_online(const float* x, int V, float& m, float& z) {
  const int tid = threadIdx.x, nvec = V >> 2, al = row_align(x);
  for (int i = tid; i < nvec; i += ST) online_acc4(load4(x + 4 * i, al), m, z);
  if (tid < V - 4 * nvec) online_acc(x[4 * nvec + tid], m, z);
}

__global__ __launch_bounds__(ST) void logits_guidance_kernel(float* cond, int64_t ld_cond, const float* uncond, int64_t ld_uncond,
                                                             int V, float scale, float log_min_p) {
  __shared__ float shf[ST / 64];
  const int tid = threadIdx.x;
  float* xc = cond + (int64_t)blockIdx.x * ld_cond;
  const float* xu = uncond + (int64_t)blockIdx.x * ld_uncond;
  float mc = -INFINITY, zc = 0.f, mu = -INFINITY, zu = 0.f;
  row_online(xc, V, mc, zc);
  row_online(xu, V, mu, zu);
  const float Mc = blk_max(mc, shf), Mu = blk_max(mu, shf);
  const float lc = logf(blk_sum(mc > -INFINITY ? zc * expf(mc - Mc) : 0.f, shf));
  const float lu = logf(blk_sum(mu > -INFINITY ? zu * expf(mu - Mu) : 0.f, shf));
  // (the barriers of the reductions stand between every read above and every write below)
  auto guide = [&](float c, float u) -> float {
    const float d = c - Mc;
    if (c == -INFINITY || d < log_min_p) return -INFINITY;       // a conditional -inf stays; the cut is on the raw logits
    const float lpc = d - lc, lpu = (u - Mu) - lu;
    return lpu + scale * (lpc - lpu);
  };
  const int nvec = V >> 2, alc = row_align(xc), alu = row_align(xu);
  for (int i = tid; i < nvec; i += ST) {
    float4 c = load4(xc + 4 * i, alc);
    const float4 u = load4(xu + 4 * i, alu);
    c.x = guide(c.x, u.x); c.y = guide(c.y, u.y); c.z = guide(c.z, u.z); c.w = guide(c.w, u.w);
    store4(xc + 4 * i, alc, c);
  }
  if (tid < V - 4 * nvec) xc[4 * nvec + tid] = guide(xc[4 * nvec + tid], xu[4 * nvec + tid]);
}

// The negative half of a guided batch follows the guided half: after the bookkeeping launch (a finished row's pad id included)
// token[R + r] = token[r], and row R + r's KV write position advances as row r's did.
__global__ void guidance_follow_kernel(int64_t* __restrict__ token, int32_t* __restrict__ d_pos, int R, int delta) {
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    token[R + r] = token[r];
    if (d_pos) d_pos[R + r] += delta;
  }
}

// Logits processors (DESIGN.md "Logits processors"): the rules of transformers' RepetitionPenaltyLogitsProcessor,
// NoRepeatNGramLogitsProcessor, MinNewTokensLengthLogitsProcessor and SuppressTokensLogitsProcessor, in that order, restated on the
// host in magma_amd/sampling.py (process_logits), as ONE enqueue-only launch in front of the selection launch: one workgroup per
// row, in place on the row's fp32 logits, reading the step from state[0] and the row's tokens so far from the history the
// bookkeeping launches keep (beam search: gathered by parent every step).  Work per row is O(step) -- history tokens, windows,
// suppress ids -- plus, for the penalty, clearing a V-bit map in LDS; only normalize = 1 (beam search: the rules apply to
// log_softmax, not renormalised) sweeps the row, with beam_topk_body's own max / logsumexp arithmetic.
struct ProcessParams {
  float* x; int64_t ld; int V;
  const int32_t* state;                     // device: [0] = step = tokens generated so far
  const int64_t* history; int64_t ld_hist; int hist_cols;
  float penalty; int ngram; int min_new; int64_t eos;
  const int32_t* suppress; int n_suppress;
  int normalize;
  const int32_t* eos_more; int n_eos_more;   // further eos ids of the min-new-tokens rule (per-row stopping with an eos list)
};

// the plain history of the launch's row: tokens [0, min(state[0], hist_cols)) from column 0
MG_DEV HistView<false> flat_view(const ProcessParams& p) {
  return HistView<false>{p.history + (int64_t)blockIdx.x * p.ld_hist, 0, max(0, min(p.state[0], p.hist_cols)), p.hist_cols};
}

// the rules of one row over its tokens h, ``step`` = the count min_new_tokens compares; ``seen``: V bits of LDS (only when the
// penalty applies): token already penalised
template <class H>
MG_DEV void process_rules(const ProcessParams p, const H h, const int step, uint32_t* seen, float* shf) {
  const int tid = threadIdx.x, V = p.V;
  float* x = p.x + (int64_t)blockIdx.x * p.ld;
  const int len = h.len;

  if (p.normalize) {
    float mx = -INFINITY;
    for (int i = tid; i < V; i += ST) mx = fmaxf(mx, x[i]);
    mx = blk_max(mx, shf);
    float z = 0.f;
    for (int i = tid; i < V; i += ST) z += expf(x[i] - mx);
    z = blk_sum(z, shf);
    const float lse = logf(z);
    for (int i = tid; i < V; i += ST) x[i] = (x[i] - mx) - lse;
    __syncthreads();
  }
  // repetition penalty, once per distinct token: the thread whose atomicOr found the token's bit clear applies it, so no
  // element is read after it was penalised, however often the token occurs
  if (p.penalty != 1.0f && len > 0) {
    for (int i = tid; i < (V + 31) / 32; i += ST) seen[i] = 0u;
    __syncthreads();
    for (int i = tid; i < len; i += ST) {
      const int64_t t = h[i];
      if (t < 0 || t >= V) continue;
      const uint32_t bit = 1u << ((int)t & 31);
      if (atomicOr(&seen[(int)t >> 5], bit) & bit) continue;
      const float v = x[t];
      x[t] = v < 0.f ? v * p.penalty : v / p.penalty;
    }
    __syncthreads();
  }
  // from here on every write is -inf and nothing is read back: no ordering between the three rules is needed
  const int n = p.ngram;
  if (n > 0 && len >= n) {
    const int pre = len - n + 1;                         // the last n - 1 tokens
    for (int w = tid; w <= len - n; w += ST) {           // one window per thread
      bool eq = true;
      for (int j = 0; j < n - 1; ++j) eq = eq && h[w + j] == h[pre + j];
      const int64_t t = h[w + n - 1];
      if (eq && t >= 0 && t < V) x[t] = -INFINITY;
    }
  }
  if (tid == 0 && step < p.min_new && p.eos >= 0 && p.eos < V) x[p.eos] = -INFINITY;
  if (tid < p.n_eos_more && step < p.min_new) {
    const int t = p.eos_more[tid];
    if (t >= 0 && t < V) x[t] = -INFINITY;
  }
  for (int i = tid; i < p.n_suppress; i += ST) {
    const int t = p.suppress[i];
    if (t >= 0 && t < V) x[t] = -INFINITY;
  }
}

__global__ __launch_bounds__(ST) void logits_process_kernel(const ProcessParams p) {
  extern __shared__ uint32_t seen[];
  __shared__ float shf[ST / 64];
  process_rules(p, flat_view(p), p.state[0], seen, shf);
}

// mg_logits_process_slots_f32: the rules over the occupant's window of the ring; an idle row keeps its bits.
struct SlotParams { const int32_t* slot; const int32_t* finish; };

__global__ __launch_bounds__(ST) void logits_process_slots_kernel(const ProcessParams p, const SlotParams s) {
  extern __shared__ uint32_t seen[];
  __shared__ float shf[ST / 64];
  const SlotWin w = slot_window(p.state, s.slot, s.finish, blockIdx.x, p.hist_cols);
  if (w.n == 0) return;                      // (uniform over the workgroup)
  process_rules(p, HistView<true>{p.history + (int64_t)blockIdx.x * p.ld_hist, w.begin, w.n, p.hist_cols}, w.n, seen, shf);
}

// Constrained decoding (DESIGN.md "Constrained decoding"; host statement: sampling.py constrain_logits; the table's layout:
// include/magma_hip.h): the same launch -- the rules above first -- then the row keeps only the tokens that continue its walk
// through a token trie.  Three phases, every loop uniform over the workgroup:
//   1. lookup    path[row][i] caches the node reached after the row's first i + 1 tokens.  It is trusted only as far as it proves
//                itself against THIS table and THIS history: thread i checks parent[path[i]] == path[i - 1] (the root for i = 0)
//                and in_token[path[i]] == history[i]; the longest prefix whose checks all pass is, by induction, the walk of that
//                prefix.  One load round trip for all 64 levels; inside a generate() loop it covers every token but the last.
//   2. walk      the tokens the prefix does not cover, one level each: the workgroup scans the node's edges for the token (one
//                round trip per 1024 edges) and records the child in path.  Inside a loop that is one level; after anything
//                else -- another call, another trie, an eager step -- as many as the cache got wrong.  Off the trie it stops.
//   3. mask      the node's edge tokens (and the eos ids, at a terminal node or off the trie) set bits in a V-bit map in LDS -- the
//                penalty's map, free again by then --, then one sweep writes -inf to every column whose bit is clear.  The sweep
//                reads no logit, so it needs no ordering against the -inf writes of the rules above.
// Every index a table entry supplies is checked against the header's counts, and the header against table_ints: a table that is
// not one leaves the eos ids only and reads nothing outside the buffer.
struct TrieParams {
  const int32_t* table; int64_t table_ints;
  const int32_t* roots;                     // [R] the root node of every row
  int32_t* path;                            // [R, MG_TRIE_MAX_LEN]
};

template <class H>
MG_DEV void constrained_body(const ProcessParams p, const TrieParams c, const H h, const int step, uint32_t* bits, float* shf) {
  __shared__ int s_good, s_child[2];
  process_rules(p, h, step, bits, shf);
  const int tid = threadIdx.x, V = p.V, row = blockIdx.x;
  float* x = p.x + (int64_t)row * p.ld;
  const int len = h.len;
  const int n = c.table[0], e = c.table[1];
  const bool sane = n >= 1 && e >= 0 && 3 + 4 * (int64_t)n + 2 * (int64_t)e <= c.table_ints;
  const int32_t* first = c.table + 2;
  const int32_t* terminal = first + (sane ? n + 1 : 0);
  const int32_t* parent = terminal + (sane ? n : 0);
  const int32_t* in_tok = parent + (sane ? n : 0);
  const int32_t* etok = in_tok + (sane ? n : 0);
  const int32_t* echild = etok + (sane ? e : 0);
  int32_t* path = c.path + (int64_t)row * MG_TRIE_MAX_LEN;
  const int root = c.roots[row];
  int cur = sane && root >= 0 && root < n ? root : -1;        // -1: off the trie
  // 1. lookup
  const int nv = cur < 0 ? 0 : min(len, MG_TRIE_MAX_LEN);
  if (tid == 0) s_good = nv;
  for (int i = tid; i < (V + 31) / 32; i += ST) bits[i] = 0u;
  __syncthreads();
  if (tid < nv) {
    const int ch = path[tid], pa = tid == 0 ? root : path[tid - 1];
    if (!(ch >= 0 && ch < n && parent[ch] == pa && (int64_t)in_tok[ch] == h[tid])) atomicMin(&s_good, tid);
  }
  __syncthreads();
  int i = s_good;
  if (i > 0) cur = path[i - 1];
  // 2. walk (s_child alternates between two slots: a slot is reset two barriers after its last reader)
  for (int it = 0; cur >= 0 && i < len; ++it) {
    const int lo = max(first[cur], 0), hi = min(first[cur + 1], e);
    if (tid == 0) s_child[it & 1] = -1;
    __syncthreads();
    const int64_t t = h[i];
    for (int j = lo + tid; j < hi; j += ST)
      if ((int64_t)etok[j] == t) s_child[it & 1] = echild[j];
    __syncthreads();
    const int ch = s_child[it & 1];
    if (ch < 0 || ch >= n || i >= MG_TRIE_MAX_LEN) { cur = -1; break; }
    if (tid == 0) path[i] = ch;
    cur = ch;
    ++i;
  }
  // 3. mask
  if (cur >= 0) {
    const int lo = max(first[cur], 0), hi = min(first[cur + 1], e);
    for (int j = lo + tid; j < hi; j += ST) {
      const int t = etok[j];
      if (t >= 0 && t < V) atomicOr(&bits[t >> 5], 1u << (t & 31));
    }
  }
  if (cur < 0 || terminal[cur] != 0) {
    if (tid == 0 && p.eos >= 0 && p.eos < V) atomicOr(&bits[(int)p.eos >> 5], 1u << ((int)p.eos & 31));
    if (tid >= 1 && tid <= p.n_eos_more) {
      const int t = p.eos_more[tid - 1];
      if (t >= 0 && t < V) atomicOr(&bits[t >> 5], 1u << (t & 31));
    }
  }
  __syncthreads();
  for (int v = tid; v < V; v += ST)
    if (!((bits[v >> 5] >> (v & 31)) & 1u)) x[v] = -INFINITY;
}

__global__ __launch_bounds__(ST) void logits_process_constrained_kernel(const ProcessParams p, const TrieParams c) {
  extern __shared__ uint32_t bits[];
  __shared__ float shf[ST / 64];
  constrained_body(p, c, flat_view(p), p.state[0], bits, shf);
}

// mg_logits_process_constrained_slots_f32: rules and trie walk over the occupant's window.  path[row] proves itself against the
// window's tokens, so what a previous occupant (or another table) left there fails the proof and the walk starts at the root.
__global__ __launch_bounds__(ST) void logits_process_constrained_slots_kernel(const ProcessParams p, const TrieParams c,
                                                                              const SlotParams s) {
  extern __shared__ uint32_t bits[];
  __shared__ float shf[ST / 64];
  const SlotWin w = slot_window(p.state, s.slot, s.finish, blockIdx.x, p.hist_cols);
  if (w.n == 0) return;                      // (uniform over the workgroup)
  constrained_body(p, c, HistView<true>{p.history + (int64_t)blockIdx.x * p.ld_hist, w.begin, w.n, p.hist_cols}, w.n, bits, shf);
}

struct BeamArgs {
  const float* cand_score; const int32_t* cand_tok;
  int B, k, K2, V; int64_t eos; double length_penalty; int early_stopping; int max_steps;
  int32_t* state; int32_t* d_pos; int n_pos;
  mg_beam_state s;
  int G; float diversity;     // grouped instance only: num_beam_groups and lambda; K2 is then the per-row list length k + k / G
};

MG_DEV bool key_before(uint32_t ka, int ia, uint32_t kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// Diverse beam search: a candidate's score less lambda times the number n of running beams of the sample's earlier groups that
// selected its token at this step -- one rounded product, one rounded subtraction, never contracted into an fma (the host
// statement, sampling.group_beam_search, rounds twice)
MG_DEV float diversity_score(float score, float lambda, int n) {
#pragma clang fp contract(off)
  const float pen = lambda * (float)n;
  return score - pen;
}

// ONE body for beam search and diverse beam search (DESIGN.md "Diverse beam search").  A group is a pseudo-sample of kq = k / G
// beams: pseudo-sample ps = smp * G + g owns rows [r0, r0 + kq), r0 = smp * k + g * kq, its own finished slots, its own unsat
// latch.  !GROUPED is G = 1 (kq = k, lists of 2k entries read from global memory as they are): beam_finish_kernel as it was.
// GROUPED: the kq lists of KL = k + kq entries are first penalised into LDS against the tokens that the sample's groups 0 .. g-1
// selected at this step (prev_tok), then merged to the top 2kq like any sample's.
template <bool GROUPED>
MG_DEV void beam_finish_body(const BeamArgs& a) {
  __shared__ int s_step, s_stopped;
  __shared__ float t_score[BK2_MAX];
  __shared__ int t_beam[BK2_MAX], t_tok[BK2_MAX];
  __shared__ int r_sel[BK_MAX];           // running row q of this (pseudo-)sample continues top candidate r_sel[q]
  __shared__ int f_src[BK_MAX];           // finished slot q: old slot f_src[q] (>= 0) or top candidate -(f_src[q] + 1)
  __shared__ int g_unsat, g_allfin, g_allhit;
  // thread 0's working set (LDS, not private arrays: dynamically indexed private arrays would live in scratch)
  __shared__ bool hit[BK2_MAX], fl[BK_MAX + BK2_MAX];
  __shared__ float mod[BK2_MAX], val[BK_MAX + BK2_MAX];
  __shared__ int pick[BK_MAX], olen[BK_MAX];
  // GROUPED: the group's penalised candidates and the tokens the sample's earlier groups selected at this step
  __shared__ float p_score[GROUPED ? 512 : 1];
  __shared__ int p_flat[GROUPED ? 512 : 1], p_tok[GROUPED ? 512 : 1];
  __shared__ int prev_tok[BK_MAX];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int R = a.B * a.k;
  const int G = GROUPED ? a.G : 1;
  const int k = GROUPED ? a.k / G : a.k;          // beams of a (pseudo-)sample
  const int K2 = 2 * k;                           // its top list
  const int KL = GROUPED ? a.K2 : K2;             // entries of a row's candidate list
  const int64_t ld = a.s.ld;
  if (tid == 0) { s_step = a.state[0]; s_stopped = a.state[1] >= 0; g_unsat = 0; g_allfin = 1; g_allhit = 1; }
  __syncthreads();
  const int step = s_step;
  if (s_stopped) {
    // generation stopped at an earlier step (the host reads the record only every few steps): the finished slots are final,
    // so nothing is selected or merged any more; identity parents make the reorder launches copy nothing
    for (int r = tid; r < R; r += nt) a.s.parent[r] = r;
    if (a.d_pos)
      for (int b = tid; b < a.n_pos; b += nt) a.d_pos[b] += 1;
    if (tid == 0) a.state[0] = step + 1;
    return;
  }
  const int cols = min(step, (int)ld);      // columns [0, step) hold the tokens of the steps so far
  for (int64_t e = tid; e < (int64_t)R * cols; e += nt) {
    const int64_t rr = e / cols, c = e % cols;
    a.s.hist_stage[rr * ld + c] = a.s.hist[rr * ld + c];
    a.s.fin_stage[rr * ld + c] = a.s.fin_tok[rr * ld + c];
  }
  __syncthreads();
  const int gen_len = step + 1;
  const float den = (float)pow((double)gen_len, a.length_penalty);
  for (int smp = 0; smp < a.B * G; ++smp) {
    const int g = GROUPED ? smp % G : 0;
    const int r0 = GROUPED ? (smp / G) * a.k + g * k : smp * k;
    // ---- top 2k of the (pseudo-)sample's k*V candidates: merge of the per-row lists ----
    if constexpr (GROUPED) {
      if (tid < k * KL) {
        const int tok = a.cand_tok[(int64_t)r0 * KL + tid];
        int n = 0;
        for (int u = 0; u < g * k; ++u) n += prev_tok[u] == tok ? 1 : 0;
        p_score[tid] = diversity_score(a.cand_score[(int64_t)r0 * KL + tid], a.diversity, n);
        p_tok[tid] = tok;
        p_flat[tid] = (tid / KL) * a.V + tok;
      }
      __syncthreads();
    }
    if (tid < k * KL) {
      const int bm = tid / KL;
      float sc; int tok;
      if constexpr (GROUPED) { sc = p_score[tid]; tok = p_tok[tid]; }
      else { sc = a.cand_score[(int64_t)r0 * KL + tid]; tok = a.cand_tok[(int64_t)r0 * KL + tid]; }
      const uint32_t kk = fkey(sc);
      const int flat = bm * a.V + tok;
      int rank = 0;
      for (int u = 0; u < k * KL; ++u) {
        if constexpr (GROUPED) rank += key_before(fkey(p_score[u]), p_flat[u], kk, flat) ? 1 : 0;
        else {
          const int bu = u / KL;
          rank += key_before(fkey(a.cand_score[(int64_t)r0 * KL + u]), bu * a.V + a.cand_tok[(int64_t)r0 * KL + u], kk, flat) ? 1 : 0;
        }
      }
      if (rank < K2) { t_score[rank] = sc; t_beam[rank] = bm; t_tok[rank] = tok; }
    }
    __syncthreads();
    if (tid == 0) {
      bool allhit = true;
      for (int j = 0; j < K2; ++j) { hit[j] = t_tok[j] == a.eos || gen_len >= a.max_steps; allhit = allhit && hit[j]; }
      // next running beams: the best k after every candidate that hit a stopping criterion lost 1e9
      for (int j = 0; j < K2; ++j) mod[j] = hit[j] ? t_score[j] + -1.0e9f : t_score[j];
      for (int j = 0; j < K2; ++j) {
        int rank = 0;
        for (int u = 0; u < K2; ++u) rank += key_before(fkey(mod[u]), u, fkey(mod[j]), j) ? 1 : 0;
        if (rank < k) r_sel[rank] = j;
      }
      for (int q = 0; q < k; ++q) {
        const int j = r_sel[q];
        a.s.run[r0 + q] = mod[j];
        a.s.parent[r0 + q] = r0 + t_beam[j];
        a.s.token[r0 + q] = t_tok[j];
        if constexpr (GROUPED) prev_tok[g * k + q] = t_tok[j];
      }
      // finished slots: merge the old k with the first k candidates that just finished
      bool full = true;
      for (int q = 0; q < k; ++q) {
        val[q] = a.s.fin_score[r0 + q]; fl[q] = a.s.fin_flag[r0 + q] != 0; olen[q] = a.s.fin_len[r0 + q];
        full = full && fl[q];
      }
      full = full && a.early_stopping == 1;
      const bool unsat = a.s.unsat[smp] != 0;
      for (int j = 0; j < K2; ++j) {
        const bool just = hit[j] && j < k;
        float v = t_score[j] / den;
        if (full) v = v + -1.0e9f;
        if (!unsat) v = v + -1.0e9f;
        if (!just) v = v + -1.0e9f;
        val[k + j] = v; fl[k + j] = just;
      }
      const int nm = k + K2;
      for (int e = 0; e < nm; ++e) {
        int rank = 0;
        for (int u = 0; u < nm; ++u) rank += key_before(fkey(val[u]), u, fkey(val[e]), e) ? 1 : 0;
        if (rank < k) pick[rank] = e;
      }
      bool allfin = true;
      float minf = INFINITY;
      for (int q = 0; q < k; ++q) {
        const int e = pick[q];
        a.s.fin_score[r0 + q] = val[e];
        a.s.fin_flag[r0 + q] = fl[e] ? 1 : 0;
        a.s.fin_len[r0 + q] = e < k ? olen[e] : gen_len;
        f_src[q] = e < k ? e : -(e - k + 1);
        allfin = allfin && fl[e];
        minf = fminf(minf, val[e]);
      }
      // early-stop heuristic on the new state (latched)
      const int hyp = (a.early_stopping == 2 && a.length_penalty > 0.0) ? a.max_steps : gen_len;
      const float best = a.s.run[r0] / (float)pow((double)hyp, a.length_penalty);
      bool any = false;
      for (int q = 0; q < k; ++q) any = any || best > (fl[pick[q]] ? minf : -1.0e9f);
      const bool unsat_new = unsat && any;
      a.s.unsat[smp] = unsat_new ? 1 : 0;
      if (unsat_new) g_unsat = 1;
      if (!allfin) g_allfin = 0;
      if (!allhit) g_allhit = 0;
    }
    __syncthreads();
    // ---- token rows: running histories gathered by parent, finished rows from the old slots or the new candidates ----
    const int w = cols + 1;
    for (int e = tid; e < 2 * k * w; e += nt) {
      const int which = e / (k * w), q = (e / w) % k, c = e % w;
      if (c >= ld) continue;
      int64_t v;
      if (which == 0) {
        const int j = r_sel[q];
        v = c < cols ? a.s.hist_stage[(int64_t)(r0 + t_beam[j]) * ld + c] : (int64_t)t_tok[j];
        a.s.hist[(int64_t)(r0 + q) * ld + c] = v;
      } else {
        const int src = f_src[q];
        if (src >= 0) v = c < cols ? a.s.fin_stage[(int64_t)(r0 + src) * ld + c] : a.eos;
        else {
          const int j = -src - 1;
          v = c < cols ? a.s.hist_stage[(int64_t)(r0 + t_beam[j]) * ld + c] : (int64_t)t_tok[j];
        }
        a.s.fin_tok[(int64_t)(r0 + q) * ld + c] = v;
      }
    }
    __syncthreads();
  }
  if (a.d_pos)
    for (int b = tid; b < a.n_pos; b += nt) a.d_pos[b] += 1;
  if (tid == 0) {
    const bool go_on = g_unsat && !(g_allfin && a.early_stopping == 1) && !g_allhit;
    if (!go_on && a.state[1] < 0) a.state[1] = step;
    a.state[0] = step + 1;
  }
}

__global__ __launch_bounds__(512) void beam_finish_kernel(const BeamArgs a) { beam_finish_body<false>(a); }
__global__ __launch_bounds__(512) void beam_finish_groups_kernel(const BeamArgs a) { beam_finish_body<true>(a); }

// grid (H, R, L); phase 0 stages the rows that must be (their own d_pos positions), phase 1 copies every non-identity row b
// from its parent p: positions [0, d_pos_p) -- what was staged of p, and in beam search d_pos_p == d_pos_b (same sample)
__global__ __launch_bounds__(256) void kv_reorder_kernel(uint4* __restrict__ kc, uint4* __restrict__ vc, uint4* __restrict__ ks,
                                                         uint4* __restrict__ vs, int R, int H, int Smax,
                                                         const int32_t* __restrict__ parent, const int32_t* __restrict__ d_pos,
                                                         int pos_stride, int phase) {
  const int h = blockIdx.x, b = blockIdx.y, l = blockIdx.z;
  auto staged = [&](int row) -> bool {           // row is overwritten and some other row reads it
    const int pr = parent[row];
    if (pr == row || pr < 0 || pr >= R) return false;      // (a row with a parent outside [0, R) is skipped, hence never overwritten:
    for (int c = 0; c < R; ++c) if (c != row && parent[c] == row) return true;     //  its readers take it from the cache itself)
    return false;
  };
  const int p = parent[b];
  if (p < 0 || p >= R) return;                   // written by the bookkeeping launch; never trusted here
  int n = d_pos[(phase == 0 ? b : p) * pos_stride];
  n = max(0, min(n, Smax));
  const int64_t per = (int64_t)256 * 2 / 16;     // uint4 per position (256 bf16)
  const int64_t cnt = (int64_t)n * per;
  if (phase == 0) {
    if (!staged(b)) return;
    const int64_t off = (((int64_t)l * R + b) * H + h) * Smax * per;
    for (int64_t i = threadIdx.x; i < cnt; i += blockDim.x) { ks[off + i] = kc[off + i]; vs[off + i] = vc[off + i]; }
  } else {
    if (p == b) return;
    const bool from_stage = staged(p);
    const int64_t dst = (((int64_t)l * R + b) * H + h) * Smax * per;
    const int64_t src = (((int64_t)l * R + p) * H + h) * Smax * per;
    const uint4* sk = from_stage ? ks : kc;
    const uint4* sv = from_stage ? vs : vc;
    for (int64_t i = threadIdx.x; i < cnt; i += blockDim.x) { kc[dst + i] = sk[src + i]; vc[dst + i] = sv[src + i]; }
  }
}

}  // namespace

extern "C" int mg_beam_topk_f32(const float* logits, int64_t ld, int32_t R, int32_t V, const float* run, int32_t K2,
                                float* cand_score, int32_t* cand_tok, void* stream) {
  if (!logits || !run || !cand_score || !cand_tok || R <= 0 || V <= 0 || ld < V)
    MG_FAIL(MG_ERR_SHAPE, "mg_beam_topk_f32: bad logits / R / V / ld");
  if (K2 < 2 || K2 > BK2_MAX || K2 > V) MG_FAIL(MG_ERR_SHAPE, "mg_beam_topk_f32: need 2 <= K2 <= min(%d, V), got %d", BK2_MAX, K2);
  hipLaunchKernelGGL(beam_topk_kernel, dim3(R), dim3(ST), 0, (hipStream_t)stream, logits, ld, V, run, K2, cand_score, cand_tok);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_beam_topk_scores_f32(const float* scores, int64_t ld, int32_t R, int32_t V, const float* run, int32_t K2,
                                       float* cand_score, int32_t* cand_tok, void* stream) {
  if (!scores || !run || !cand_score || !cand_tok || R <= 0 || V <= 0 || ld < V)
    MG_FAIL(MG_ERR_SHAPE, "mg_beam_topk_scores_f32: bad scores / R / V / ld");
  if (K2 < 2 || K2 > BK2_MAX || K2 > V) MG_FAIL(MG_ERR_SHAPE, "mg_beam_topk_scores_f32: need 2 <= K2 <= min(%d, V), got %d", BK2_MAX, K2);
  hipLaunchKernelGGL(beam_topk_pre_kernel, dim3(R), dim3(ST), 0, (hipStream_t)stream, scores, ld, V, run, K2, cand_score, cand_tok);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_token_logprobs_f32(const float* logits, int64_t ld, int32_t R, int32_t V, const int64_t* token,
                                     const int32_t* state, float* lp, int64_t ld_lp, int32_t cols, int32_t n_top, int32_t* top_id,
                                     float* top_lp, void* stream) {
  if (!logits || !token || !lp || R <= 0 || V <= 0 || ld < V) MG_FAIL(MG_ERR_SHAPE, "mg_token_logprobs_f32: bad logits / token / lp / R / V / ld");
  if (cols < 1 || ld_lp < cols) MG_FAIL(MG_ERR_SHAPE, "mg_token_logprobs_f32: need 1 <= cols <= ld_lp, got %d / %lld", cols, (long long)ld_lp);
  if (n_top < 0 || n_top > MG_LOGPROBS_MAX_TOP || n_top > V)
    MG_FAIL(MG_ERR_SHAPE, "mg_token_logprobs_f32: need 0 <= n_top <= min(%d, V), got %d (V = %d)", MG_LOGPROBS_MAX_TOP, n_top, V);
  if (n_top > 0 && (!top_id || !top_lp)) MG_FAIL(MG_ERR_SHAPE, "mg_token_logprobs_f32: n_top > 0 needs top_id and top_lp");
  static_assert(MG_LOGPROBS_MAX_TOP <= BK2_MAX, "the top lists are collected in row_topk_body's slots");
  hipLaunchKernelGGL(token_logprobs_kernel, dim3(R), dim3(ST), 0, (hipStream_t)stream, logits, ld, V, token, state, lp, ld_lp, cols,
                     n_top, n_top > 0 ? top_id : nullptr, n_top > 0 ? top_lp : nullptr);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_token_logprobs_slots_f32(const float* logits, int64_t ld, int32_t R, int32_t V, const int64_t* token,
                                           const int32_t* state, float* lp, int64_t ld_lp, int32_t cols, int32_t n_top,
                                           int32_t* top_id, float* top_lp, const int32_t* slot, const int32_t* finish,
                                           int32_t history_cols, void* stream) {
  const char* who = "mg_token_logprobs_slots_f32";
  if (!logits || !token || !lp || R <= 0 || V <= 0 || ld < V) MG_FAIL(MG_ERR_SHAPE, "%s: bad logits / token / lp / R / V / ld", who);
  if (!state || !slot || !finish || history_cols < 1)
    MG_FAIL(MG_ERR_SHAPE, "%s: needs state, slot [R][2], finish [R][2] and history_cols >= 1 (the ring the windows lie in)", who);
  if (cols < 1 || ld_lp < cols) MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= cols <= ld_lp, got %d / %lld", who, cols, (long long)ld_lp);
  if (n_top < 0 || n_top > MG_LOGPROBS_MAX_TOP || n_top > V)
    MG_FAIL(MG_ERR_SHAPE, "%s: need 0 <= n_top <= min(%d, V), got %d (V = %d)", who, MG_LOGPROBS_MAX_TOP, n_top, V);
  if (n_top > 0 && (!top_id || !top_lp)) MG_FAIL(MG_ERR_SHAPE, "%s: n_top > 0 needs top_id and top_lp", who);
  hipLaunchKernelGGL(token_logprobs_slots_kernel, dim3(R), dim3(ST), 0, (hipStream_t)stream, logits, ld, V, token, state, lp, ld_lp,
                     cols, n_top, n_top > 0 ? top_id : nullptr, n_top > 0 ? top_lp : nullptr, slot, finish, history_cols);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_logits_guidance_f32(float* cond, int64_t ld_cond, const float* uncond, int64_t ld_uncond, int32_t R, int32_t V,
                                      float scale, float log_min_p, void* stream) {
  if (!cond || !uncond || R <= 0 || V <= 0 || ld_cond < V || ld_uncond < V)
    MG_FAIL(MG_ERR_SHAPE, "mg_logits_guidance_f32: bad cond / uncond / R / V / ld");
  if (!(scale >= 0.f) || scale == INFINITY) MG_FAIL(MG_ERR_SHAPE, "mg_logits_guidance_f32: scale must be finite and >= 0");
  if (!(log_min_p <= 0.f)) MG_FAIL(MG_ERR_SHAPE, "mg_logits_guidance_f32: log_min_p must be <= 0 (-inf: no cut)");
  hipLaunchKernelGGL(logits_guidance_kernel, dim3(R), dim3(ST), 0, (hipStream_t)stream, cond, ld_cond, uncond, ld_uncond, V, scale,
                     log_min_p);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_guidance_follow(int64_t* token, int32_t* d_pos, int32_t R, int32_t delta, int32_t pos_stride, void* stream) {
  if (!token || R <= 0) MG_FAIL(MG_ERR_SHAPE, "mg_guidance_follow: bad arguments");
  if (pos_stride != 0 && pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "mg_guidance_follow: pos_stride must be 0 or 1");
  hipLaunchKernelGGL(guidance_follow_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, token, pos_stride ? d_pos : nullptr, R, delta);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

// the checks mg_logits_process_f32 and mg_logits_process_constrained_f32 share
static int process_args_check(const char* fn, const float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* state,
                              const int64_t* history, int64_t ld_history, int32_t history_cols, float repetition_penalty,
                              int32_t no_repeat_ngram, int32_t min_new_tokens, const int32_t* suppress, int32_t n_suppress,
                              const int32_t* eos_more, int32_t n_eos_more, bool reads_history, bool uses_map) {
  if (!logits || !state || R <= 0 || V <= 0 || ld < V) MG_FAIL(MG_ERR_SHAPE, "%s: bad logits / state / R / V / ld", fn);
  if (!(repetition_penalty > 0.f)) MG_FAIL(MG_ERR_SHAPE, "%s: repetition_penalty must be > 0", fn);
  if (no_repeat_ngram < 0 || no_repeat_ngram > 16 || min_new_tokens < 0)
    MG_FAIL(MG_ERR_SHAPE, "%s: need 0 <= no_repeat_ngram <= 16 and min_new_tokens >= 0", fn);
  if (n_suppress < 0 || n_suppress > 1024 || (n_suppress > 0 && !suppress))
    MG_FAIL(MG_ERR_SHAPE, "%s: need 0 <= n_suppress <= 1024 and a suppress array", fn);
  if (n_eos_more < 0 || n_eos_more > MG_STOP_MAX_EOS || (n_eos_more > 0 && !eos_more))
    MG_FAIL(MG_ERR_SHAPE, "%s: need 0 <= n_eos_more <= %d and an eos_more array", fn, MG_STOP_MAX_EOS);
  if (reads_history && (!history || history_cols <= 0 || ld_history < history_cols))
    MG_FAIL(MG_ERR_SHAPE, "%s: the penalty, the n-gram rule and the constraint need a history [R, ld_history >= history_cols > 0]", fn);
  if (uses_map && (size_t)((V + 31) / 32) * 4 > 60 * 1024)
    MG_FAIL(MG_ERR_SHAPE, "%s: V = %d exceeds the LDS token map (491 520 tokens)", fn, V);
  return MG_OK;
}

extern "C" int mg_logits_process_f32(float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* state, const int64_t* history,
                                     int64_t ld_history, int32_t history_cols, float repetition_penalty, int32_t no_repeat_ngram,
                                     int32_t min_new_tokens, int64_t eos, const int32_t* suppress, int32_t n_suppress,
                                     int32_t normalize, const int32_t* eos_more, int32_t n_eos_more, void* stream) {
  const int rc = process_args_check("mg_logits_process_f32", logits, ld, R, V, state, history, ld_history, history_cols,
                                    repetition_penalty, no_repeat_ngram, min_new_tokens, suppress, n_suppress, eos_more, n_eos_more,
                                    repetition_penalty != 1.0f || no_repeat_ngram > 0, repetition_penalty != 1.0f);
  if (rc != MG_OK) return rc;
  const size_t lds = repetition_penalty != 1.0f ? (size_t)((V + 31) / 32) * 4 : 0;
  ProcessParams p{logits, ld, V, state, history, ld_history, history ? history_cols : 0, repetition_penalty, no_repeat_ngram,
                  min_new_tokens, eos, suppress, n_suppress, normalize ? 1 : 0, eos_more, eos_more ? n_eos_more : 0};
  hipLaunchKernelGGL(logits_process_kernel, dim3(R), dim3(ST), lds, (hipStream_t)stream, p);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_logits_process_constrained_f32(float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* state,
                                                 const int64_t* history, int64_t ld_history, int32_t history_cols,
                                                 float repetition_penalty, int32_t no_repeat_ngram, int32_t min_new_tokens,
                                                 int64_t eos, const int32_t* suppress, int32_t n_suppress, const int32_t* eos_more,
                                                 int32_t n_eos_more, const int32_t* table, int64_t table_ints, const int32_t* roots,
                                                 int32_t* path, void* stream) {
  const int rc = process_args_check("mg_logits_process_constrained_f32", logits, ld, R, V, state, history, ld_history, history_cols,
                                    repetition_penalty, no_repeat_ngram, min_new_tokens, suppress, n_suppress, eos_more, n_eos_more,
                                    true, true);
  if (rc != MG_OK) return rc;
  if (!table || table_ints < 2 || !roots || !path)
    MG_FAIL(MG_ERR_SHAPE, "mg_logits_process_constrained_f32: need a table of at least 2 ints, roots [R] and path [R, %d]", MG_TRIE_MAX_LEN);
  ProcessParams p{logits, ld, V, state, history, ld_history, history_cols, repetition_penalty, no_repeat_ngram,
                  min_new_tokens, eos, suppress, n_suppress, 0, eos_more, eos_more ? n_eos_more : 0};
  TrieParams c{table, table_ints, roots, path};
  hipLaunchKernelGGL(logits_process_constrained_kernel, dim3(R), dim3(ST), (size_t)((V + 31) / 32) * 4, (hipStream_t)stream, p, c);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_logits_process_slots_f32(float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* state,
                                           const int64_t* history, int64_t ld_history, int32_t history_cols,
                                           float repetition_penalty, int32_t no_repeat_ngram, int32_t min_new_tokens, int64_t eos,
                                           const int32_t* suppress, int32_t n_suppress, int32_t normalize, const int32_t* eos_more,
                                           int32_t n_eos_more, const int32_t* slot, const int32_t* finish, void* stream) {
  // (the window's length needs the ring's column count whatever the rules are: the history is never optional here)
  const int rc = process_args_check("mg_logits_process_slots_f32", logits, ld, R, V, state, history, ld_history, history_cols,
                                    repetition_penalty, no_repeat_ngram, min_new_tokens, suppress, n_suppress, eos_more, n_eos_more,
                                    true, repetition_penalty != 1.0f);
  if (rc != MG_OK) return rc;
  if (!slot || !finish) MG_FAIL(MG_ERR_SHAPE, "mg_logits_process_slots_f32: need slot [R][2] and finish [R][2]");
  const size_t lds = repetition_penalty != 1.0f ? (size_t)((V + 31) / 32) * 4 : 0;
  ProcessParams p{logits, ld, V, state, history, ld_history, history_cols, repetition_penalty, no_repeat_ngram,
                  min_new_tokens, eos, suppress, n_suppress, normalize ? 1 : 0, eos_more, eos_more ? n_eos_more : 0};
  hipLaunchKernelGGL(logits_process_slots_kernel, dim3(R), dim3(ST), lds, (hipStream_t)stream, p, SlotParams{slot, finish});
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_logits_process_constrained_slots_f32(float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* state,
                                                       const int64_t* history, int64_t ld_history, int32_t history_cols,
                                                       float repetition_penalty, int32_t no_repeat_ngram, int32_t min_new_tokens,
                                                       int64_t eos, const int32_t* suppress, int32_t n_suppress,
                                                       const int32_t* eos_more, int32_t n_eos_more, const int32_t* table,
                                                       int64_t table_ints, const int32_t* roots, int32_t* path, const int32_t* slot,
                                                       const int32_t* finish, void* stream) {
  const char* who = "mg_logits_process_constrained_slots_f32";
  const int rc = process_args_check(who, logits, ld, R, V, state, history, ld_history, history_cols, repetition_penalty,
                                    no_repeat_ngram, min_new_tokens, suppress, n_suppress, eos_more, n_eos_more, true, true);
  if (rc != MG_OK) return rc;
  if (!table || table_ints < 2 || !roots || !path)
    MG_FAIL(MG_ERR_SHAPE, "%s: need a table of at least 2 ints, roots [R] and path [R, %d]", who, MG_TRIE_MAX_LEN);
  if (!slot || !finish) MG_FAIL(MG_ERR_SHAPE, "%s: need slot [R][2] and finish [R][2]", who);
  ProcessParams p{logits, ld, V, state, history, ld_history, history_cols, repetition_penalty, no_repeat_ngram,
                  min_new_tokens, eos, suppress, n_suppress, 0, eos_more, eos_more ? n_eos_more : 0};
  TrieParams c{table, table_ints, roots, path};
  hipLaunchKernelGGL(logits_process_constrained_slots_kernel, dim3(R), dim3(ST), (size_t)((V + 31) / 32) * 4, (hipStream_t)stream, p,
                     c, SlotParams{slot, finish});
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_beam_finish(const float* cand_score, const int32_t* cand_tok, int32_t B, int32_t k, int32_t V, int64_t eos,
                              double length_penalty, int32_t early_stopping, int32_t max_steps, int32_t* state, int32_t* d_pos,
                              int32_t pos_stride, const mg_beam_state* bs, void* stream) {
  if (!cand_score || !cand_tok || !state || !bs || B <= 0 || k < 1 || k > BK_MAX || V < 2 * k || max_steps < 1)
    MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish: bad arguments (B %d, k %d, V %d, max_steps %d)", B, k, V, max_steps);
  if (early_stopping < 0 || early_stopping > 2) MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish: early_stopping must be 0, 1 or 2");
  if (pos_stride != 0 && pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish: pos_stride must be 0 or 1");
  const mg_beam_state& s = *bs;
  if (!s.run || !s.fin_score || !s.fin_flag || !s.fin_len || !s.fin_tok || !s.fin_stage || !s.hist || !s.hist_stage ||
      !s.unsat || !s.parent || !s.token || s.ld < 1)
    MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish: a beam-state buffer is missing");
  BeamArgs a{cand_score, cand_tok, B, k, 2 * k, V, eos, length_penalty, early_stopping, max_steps, state, d_pos,
             pos_stride ? B * k : 1, s, 1, 0.f};
  hipLaunchKernelGGL(beam_finish_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, a);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_beam_finish_groups(const float* cand_score, const int32_t* cand_tok, int32_t B, int32_t k, int32_t G, int32_t K2,
                                     float diversity_penalty, int32_t V, int64_t eos, double length_penalty,
                                     int32_t early_stopping, int32_t max_steps, int32_t* state, int32_t* d_pos, int32_t pos_stride,
                                     const mg_beam_state* bs, void* stream) {
  if (!cand_score || !cand_tok || !state || !bs || B <= 0 || k < 1 || k > BK_MAX || max_steps < 1)
    MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish_groups: bad arguments (B %d, k %d, max_steps %d)", B, k, max_steps);
  if (G < 1 || G > k || k % G != 0) MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish_groups: G = %d must lie in [1, k] and divide k = %d", G, k);
  const int kq = k / G;
  if (G > 1 ? K2 != k + kq : K2 != 2 * k)
    MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish_groups: K2 must be k + k / G = %d (2k at G = 1), got %d", G > 1 ? k + kq : 2 * k, K2);
  if (K2 > BK2_MAX || kq * K2 > 512 || V < K2)
    MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish_groups: need K2 <= min(%d, V) and (k / G) * K2 <= 512 (K2 %d, V %d)", BK2_MAX, K2, V);
  if (!(diversity_penalty >= 0.f) || diversity_penalty == INFINITY)      // (NaN fails the first test)
    MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish_groups: diversity_penalty must be finite and >= 0");
  if (early_stopping < 0 || early_stopping > 2) MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish_groups: early_stopping must be 0, 1 or 2");
  if (pos_stride != 0 && pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish_groups: pos_stride must be 0 or 1");
  const mg_beam_state& s = *bs;
  if (!s.run || !s.fin_score || !s.fin_flag || !s.fin_len || !s.fin_tok || !s.fin_stage || !s.hist || !s.hist_stage ||
      !s.unsat || !s.parent || !s.token || s.ld < 1)
    MG_FAIL(MG_ERR_SHAPE, "mg_beam_finish_groups: a beam-state buffer is missing");
  BeamArgs a{cand_score, cand_tok, B, k, K2, V, eos, length_penalty, early_stopping, max_steps, state, d_pos,
             pos_stride ? B * k : 1, s, G, diversity_penalty};
  hipLaunchKernelGGL(beam_finish_groups_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, a);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_kv_reorder_bf16(mg_bf16* kcache, mg_bf16* vcache, mg_bf16* kstage, mg_bf16* vstage, int32_t L, int32_t R,
                                  int32_t H, int32_t Smax, const int32_t* parent, const int32_t* d_pos, int32_t pos_stride,
                                  void* stream) {
  if (!kcache || !vcache || !kstage || !vstage || !parent || !d_pos || L <= 0 || R <= 0 || H <= 0 || Smax <= 0)
    MG_FAIL(MG_ERR_SHAPE, "mg_kv_reorder_bf16: bad arguments");
  if (pos_stride != 0 && pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "mg_kv_reorder_bf16: pos_stride must be 0 or 1");
  if (!MG_ALIGNED16(kcache) || !MG_ALIGNED16(vcache) || !MG_ALIGNED16(kstage) || !MG_ALIGNED16(vstage))
    MG_FAIL(MG_ERR_SHAPE, "mg_kv_reorder_bf16: buffers must be 16-byte aligned");
  if (H > 65535 || L > 65535) MG_FAIL(MG_ERR_SHAPE, "mg_kv_reorder_bf16: grid too large");
  for (int phase = 0; phase < 2; ++phase) {
    hipLaunchKernelGGL(kv_reorder_kernel, dim3(H, R, L), dim3(256), 0, (hipStream_t)stream, (uint4*)kcache, (uint4*)vcache,
                       (uint4*)kstage, (uint4*)vstage, R, H, Smax, parent, d_pos, pos_stride, phase);
    MG_CHECK_LAUNCH();
  }
  return MG_OK;
}

// ---------------------------------------------------------------------------
// Token log-probabilities by row index (behind everything else: the kernels of the token step keep their place in the code object)
namespace {
// mg_token_logprobs_f32 with a row indirection (mg_token_logprobs_rows_f32, ABI 19; DESIGN.md "Ranking choices"): entry i reads logits row
// row_of[i] and token[i], so the children of one trie node share their parent's logits row without a copy.  token_logprobs_kernel's
// body in its n_top = 0 form -- the same max / logsumexp, the same expression -- hence the same bits for the same row and token.
// A row outside [0, n_rows) or a token outside [0, V) reads nothing and gives -inf.
__global__ __launch_bounds__(ST) void token_logprobs_rows_kernel(const float* __restrict__ logits, int64_t ld, int n_rows, int V,
                                                                 const int32_t* __restrict__ row_of,
                                                                 const int32_t* __restrict__ token, float* __restrict__ lp) {
  const int i = blockIdx.x, row = row_of[i];
  if (row < 0 || row >= n_rows) {            // (uniform over the workgroup)
    if (threadIdx.x == 0) lp[i] = -INFINITY;
    return;
  }
  const float* x = logits + (int64_t)row * ld;
  const RowLse s = row_topk_body<false, true>(x, V, 0.f, 0, nullptr, nullptr);
  if (threadIdx.x == 0) {
    const int t = token[i];
    lp[i] = t >= 0 && t < V ? (x[t] - s.mx) - s.lse : -INFINITY;
  }
}
}  // namespace

extern "C" int mg_token_logprobs_rows_f32(const float* logits, int64_t ld, int32_t n_rows, int32_t V, const int32_t* row_of,
                                          const int32_t* token, int32_t N, float* lp, void* stream) {
  const char* who = "mg_token_logprobs_rows_f32";
  if (!logits || !row_of || !token || !lp) MG_FAIL(MG_ERR_SHAPE, "%s: null pointer", who);
  if (n_rows <= 0 || V <= 0 || N <= 0 || ld < V) MG_FAIL(MG_ERR_SHAPE, "%s: need n_rows, V, N > 0 and ld >= V", who);
  if (((uintptr_t)logits | (uintptr_t)row_of | (uintptr_t)token | (uintptr_t)lp) & 3) MG_FAIL(MG_ERR_ALIGN, "%s: pointers must be 4-byte aligned", who);
  hipLaunchKernelGGL(token_logprobs_rows_kernel, dim3(N), dim3(ST), 0, (hipStream_t)stream, logits, ld, n_rows, V, row_of, token, lp);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

// ================================================================================================================================
// Contrastive search (ABI 22; Su et al. 2022; DESIGN.md "Contrastive search"; host statement: magma_amd/sampling.py,
// contrastive_rank / contrastive_search).  A sample owns k cache rows, one per candidate token; per token step, behind the head:
//   contrastive_sim_kernel     grid (context chunks of 32 positions, samples), 8 waves: cosines of the <= 16 candidate hidden rows
//                              against the chunk's context rows on the 16x16x32 bf16 MFMA (context rows the 16-row operand, the
//                              candidates -- zero beyond k -- the 16 columns), wave w taking d / 8 of the hidden size; every lane loads 16
//                              bytes per operand and K-slice, the squared norms of both sides are summed from the very fragments
//                              the MFMA reads.  The eight partial tiles meet in LDS; per candidate the maximum over the chunk's
//                              valid positions goes to part[b, chunk, j].  Nothing is shared between workgroups.
//   contrastive_finish_kernel  one workgroup: per sample the maximum over the chunks, score_j = (1 - alpha) p_j - alpha penalty_j, the
//                              first largest j; the selected token to the history, src[b] = the selected row, its hidden row
//                              appended to the context store; then mg_sample_finish's bookkeeping (one workgroup because the
//                              all-eos latch and the step counter are the whole batch's).
//   kv_broadcast_kernel        the K / V of the selected row at the position just written, to the sample's other k - 1 rows.
//   contrastive_topk_kernel    row_topk_body's max / logsumexp / radix descent on the selected row's logits: the next k candidates
//                              (raw logit descending, lower id first) into the token rows of the sample, p = exp(log_softmax).
namespace {

constexpr int CS_CHUNK = 32;            // context positions per workgroup of the similarity kernel (MG_CONTRASTIVE_CHUNK)
constexpr int CS_WAVES = 8;
constexpr float CS_EMPTY = -1.0e30f;    // part[] of a chunk without a valid position

MG_DEV float sumsq8(const u32x4 w) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) { const float a = bflo(w[i]), b = bfhi(w[i]); s = fmaf(a, a, s); s = fmaf(b, b, s); }
  return s;
}

__global__ __launch_bounds__(CS_WAVES * 64) void contrastive_sim_kernel(const mg_bf16* __restrict__ hidden, int64_t ld_h,
                                                                        const mg_bf16* __restrict__ ctx, int Tmax, int d,
                                                                        const int32_t* __restrict__ ctx_len, int k,
                                                                        float* __restrict__ part, int n_chunk) {
  __shared__ float s_acc[CS_WAVES][2][256];
  __shared__ float s_nx[CS_WAVES][CS_CHUNK];
  __shared__ float s_nc[CS_WAVES][16];
  __shared__ float s_cos[CS_CHUNK][16];
  const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int len = max(0, min(ctx_len[b], Tmax));
  const int p0 = chunk * CS_CHUNK;
  float* out = part + ((int64_t)b * n_chunk + chunk) * k;
  if (p0 >= len) {                           // (uniform over the workgroup)
    if (tid < k) out[tid] = CS_EMPTY;
    return;
  }
  const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
  const int dw = d / CS_WAVES, kbeg = wave * dw + lq * 8;
  // rows past the valid length read the last valid row (inside the store) and are masked below
  const mg_bf16* base = ctx + (int64_t)b * Tmax * d;
  const mg_bf16* ra = base + (int64_t)min(p0 + li, len - 1) * d + kbeg;
  const mg_bf16* rb = base + (int64_t)min(p0 + 16 + li, len - 1) * d + kbeg;
  const bool cand = li < k;
  const mg_bf16* rc = hidden + ((int64_t)b * k + min(li, k - 1)) * ld_h + kbeg;
  f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
  float na = 0.f, nb = 0.f, nc = 0.f;
  auto slice = [&](const u32x4 fa, const u32x4 fb, const u32x4 fc) {
    const bf16x8 c8 = __builtin_bit_cast(bf16x8, fc);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa), c8, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fb), c8, acc1, 0, 0, 0);
    na += sumsq8(fa); nb += sumsq8(fb); nc += sumsq8(fc);
  };
  const u32x4 zero = (u32x4){0u, 0u, 0u, 0u};
  int k0 = 0;
  for (; k0 + 128 <= dw; k0 += 128) {        // four K-slices in flight: 12 loads of 16 bytes per lane
    u32x4 fa[4], fb[4], fc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      fa[u] = *(const u32x4*)(ra + k0 + 32 * u);
      fb[u] = *(const u32x4*)(rb + k0 + 32 * u);
      fc[u] = cand ? *(const u32x4*)(rc + k0 + 32 * u) : zero;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) slice(fa[u], fb[u], fc[u]);
  }
  for (; k0 < dw; k0 += 32)
    slice(*(const u32x4*)(ra + k0), *(const u32x4*)(rb + k0), cand ? *(const u32x4*)(rc + k0) : zero);
  // the four k-groups of a row sit 16 lanes apart
  na += __shfl_xor(na, 16, 64); na += __shfl_xor(na, 32, 64);
  nb += __shfl_xor(nb, 16, 64); nb += __shfl_xor(nb, 32, 64);
  nc += __shfl_xor(nc, 16, 64); nc += __shfl_xor(nc, 32, 64);
#pragma unroll
  for (int r = 0; r < 4; ++r) {              // acc[r]: context row lq * 4 + r of the tile, candidate li
    s_acc[wave][0][(lq * 4 + r) * 16 + li] = acc0[r];
    s_acc[wave][1][(lq * 4 + r) * 16 + li] = acc1[r];
  }
  if (lq == 0) { s_nx[wave][li] = na; s_nx[wave][16 + li] = nb; s_nc[wave][li] = nc; }
  __syncthreads();
  {
    const int p = tid >> 4, j = tid & 15;    // 512 threads: 32 positions x 16 candidates
    float dot = 0.f, nx = 0.f, ncj = 0.f;
#pragma unroll
    for (int w = 0; w < CS_WAVES; ++w) {
      dot += s_acc[w][p >> 4][(p & 15) * 16 + j];
      nx += s_nx[w][p];
      ncj += s_nc[w][j];
    }
    float c = (nx > 0.f && ncj > 0.f) ? dot / (sqrtf(nx) * sqrtf(ncj)) : 0.f;
    if (p0 + p >= len) c = CS_EMPTY;
    s_cos[p][j] = c;
  }
  __syncthreads();
  if (tid < k) {
    float m = CS_EMPTY;
#pragma unroll
    for (int p = 0; p < CS_CHUNK; ++p) m = fmaxf(m, s_cos[p][tid]);
    out[tid] = m;
  }
}

struct ContrastFinishArgs {
  const float* part; int n_chunk; const float* cand_p; int B, k; float alpha;
  const mg_bf16* hidden; int64_t ld_h; int d; mg_bf16* ctx; int Tmax; int32_t* ctx_len; int32_t* src;
  const int64_t* token; int64_t* history; int64_t ld_hist; int hist_cols; int64_t eos; int32_t* state;
  int32_t* d_pos; int n_pos, delta;
};

__global__ __launch_bounds__(256) void contrastive_finish_kernel(const ContrastFinishArgs a) {
  __shared__ int s_step, s_sel, s_all;
  __shared__ float s_score[BK_MAX];
  const int tid = threadIdx.x, k = a.k;
  if (tid == 0) { s_step = a.state[0]; s_all = 1; }      // read once, before thread 0 bumps it (sample_finish_kernel)
  __syncthreads();
  const int step = s_step;
  for (int b = 0; b < a.B; ++b) {
    if (tid < k) {
      float pen = CS_EMPTY;
      for (int c = 0; c < a.n_chunk; ++c) pen = fmaxf(pen, a.part[((int64_t)b * a.n_chunk + c) * k + tid]);
      if (pen <= CS_EMPTY) pen = 0.f;                    // no context position at all
      s_score[tid] = (1.f - a.alpha) * a.cand_p[b * k + tid] - a.alpha * pen;
    }
    __syncthreads();
    if (tid == 0) {
      int best = 0;
      for (int j = 1; j < k; ++j) if (s_score[j] > s_score[best]) best = j;
      s_sel = best;
    }
    __syncthreads();
    const int row = b * k + s_sel;
    const int len = a.ctx_len[b];
    const int64_t tok = a.token[row];
    if (len >= 0 && len < a.Tmax) {                      // the selected hidden row joins the context
      const uint4* s = (const uint4*)(a.hidden + (int64_t)row * a.ld_h);
      uint4* t = (uint4*)(a.ctx + ((int64_t)b * a.Tmax + len) * a.d);
      for (int i = tid; i < a.d / 8; i += blockDim.x) t[i] = s[i];
    }
    if (a.history && tid < k && step >= 0 && step < a.hist_cols) a.history[(int64_t)(b * k + tid) * a.ld_hist + step] = tok;
    __syncthreads();                                     // every thread has read ctx_len[b] and s_sel
    if (tid == 0) {
      a.src[b] = row;
      if (len >= 0 && len < a.Tmax) a.ctx_len[b] = len + 1;
      if (tok != a.eos) s_all = 0;
    }
  }
  if (a.d_pos)
    for (int i = tid; i < a.n_pos; i += blockDim.x) a.d_pos[i] += a.delta;
  __syncthreads();
  if (tid != 0) return;
  if (s_all && a.state[1] < 0) a.state[1] = step;
  a.state[0] = step + 1;
}

// grid (H, R, L), 64 threads: lanes 0-31 one 16-byte piece of the K row each, lanes 32-63 of the V row
__global__ __launch_bounds__(64) void kv_broadcast_kernel(uint4* __restrict__ kc, uint4* __restrict__ vc, int R, int H, int Smax,
                                                          int k, const int32_t* __restrict__ src,
                                                          const int32_t* __restrict__ d_pos, int pos_stride, int pos_delta) {
  const int h = blockIdx.x, r = blockIdx.y, l = blockIdx.z;
  const int b = r / k, s = src[b];
  if (s == r || s < b * k || s >= b * k + k) return;     // written by the bookkeeping launch; never trusted here
  const int pos = (int)((unsigned)d_pos[r * pos_stride] + (unsigned)pos_delta);     // (unsigned: the sum cannot overflow in front of the compare)
  if ((unsigned)pos >= (unsigned)Smax) return;
  const int64_t per = 32;                                // uint4 per position (256 bf16)
  const int64_t dst = ((((int64_t)l * R + r) * H + h) * Smax + pos) * per;
  const int64_t from = ((((int64_t)l * R + s) * H + h) * Smax + pos) * per;
  const int i = threadIdx.x & 31;
  if (threadIdx.x < 32) kc[dst + i] = kc[from + i];
  else vc[dst + i] = vc[from + i];
}

__global__ __launch_bounds__(ST) void contrastive_topk_kernel(const float* __restrict__ logits, int64_t ld, int R, int V,
                                                              const int32_t* __restrict__ src, int k, int64_t* __restrict__ token,
                                                              float* __restrict__ cand_p) {
  __shared__ float s_lp[BK2_MAX];
  __shared__ int32_t s_tok[BK2_MAX];
  const int b = blockIdx.x;
  int row = src[b];
  if (row < b * k || row >= b * k + k || row >= R) row = b * k;      // (uniform; never trusted)
  row_topk_body<false, true>(logits + (int64_t)row * ld, V, 0.f, k, s_lp, s_tok);
  __syncthreads();
  if (threadIdx.x < k) {
    token[b * k + threadIdx.x] = (int64_t)s_tok[threadIdx.x];
    cand_p[b * k + threadIdx.x] = expf(s_lp[threadIdx.x]);
  }
}

}  // namespace

extern "C" int mg_contrastive_topk_f32(const float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* src, int32_t B,
                                       int32_t k, int64_t* token, float* cand_p, void* stream) {
  const char* who = "mg_contrastive_topk_f32";
  if (!logits || !src || !token || !cand_p) MG_FAIL(MG_ERR_SHAPE, "%s: null pointer", who);
  if (B <= 0 || V <= 0 || ld < V) MG_FAIL(MG_ERR_SHAPE, "%s: need B, V > 0 and ld >= V", who);
  if (k < 1 || k > BK_MAX || k > V) MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= k <= min(%d, V), got %d (V = %d)", who, BK_MAX, k, V);
  if (R != B * k) MG_FAIL(MG_ERR_SHAPE, "%s: logits must hold R = B * k = %d rows, got %d", who, B * k, R);
  if (((uintptr_t)logits | (uintptr_t)src | (uintptr_t)cand_p) & 3) MG_FAIL(MG_ERR_ALIGN, "%s: logits, src and cand_p must be 4-byte aligned", who);
  if ((uintptr_t)token & 7) MG_FAIL(MG_ERR_ALIGN, "%s: token must be 8-byte aligned", who);
  hipLaunchKernelGGL(contrastive_topk_kernel, dim3(B), dim3(ST), 0, (hipStream_t)stream, logits, ld, R, V, src, k, token, cand_p);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_contrastive_sim_bf16(const mg_bf16* hidden, int64_t ld_hidden, const mg_bf16* ctx, int32_t B, int32_t Tmax,
                                       int32_t d, const int32_t* ctx_len, int32_t len_max, int32_t k, float* part, int32_t n_chunk,
                                       void* stream) {
  const char* who = "mg_contrastive_sim_bf16";
  if (!hidden || !ctx || !ctx_len || !part) MG_FAIL(MG_ERR_SHAPE, "%s: null pointer", who);
  if (B <= 0 || B > 65535 || Tmax <= 0) MG_FAIL(MG_ERR_SHAPE, "%s: need 0 < B <= 65535 and Tmax > 0", who);
  if (len_max < 0 || len_max > Tmax) MG_FAIL(MG_ERR_SHAPE, "%s: ctx_len reaches %d, the store holds Tmax = %d positions", who, len_max, Tmax);
  if (k < 1 || k > BK_MAX) MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= k <= %d, got %d", who, BK_MAX, k);
  if (d <= 0 || d % 256 != 0) MG_FAIL(MG_ERR_SHAPE, "%s: d must be a multiple of 256, got %d", who, d);
  if (ld_hidden < d || ld_hidden % 8 != 0) MG_FAIL(MG_ERR_SHAPE, "%s: ld_hidden must be >= d and a multiple of 8", who);
  if (n_chunk != (Tmax + CS_CHUNK - 1) / CS_CHUNK)
    MG_FAIL(MG_ERR_SHAPE, "%s: part holds n_chunk = ceil(Tmax / %d) = %d chunks per sample, got %d", who, CS_CHUNK, (Tmax + CS_CHUNK - 1) / CS_CHUNK, n_chunk);
  if (!MG_ALIGNED16(hidden) || !MG_ALIGNED16(ctx)) MG_FAIL(MG_ERR_ALIGN, "%s: hidden and ctx must be 16-byte aligned", who);
  if (((uintptr_t)ctx_len | (uintptr_t)part) & 3) MG_FAIL(MG_ERR_ALIGN, "%s: ctx_len and part must be 4-byte aligned", who);
  hipLaunchKernelGGL(contrastive_sim_kernel, dim3(n_chunk, B), dim3(CS_WAVES * 64), 0, (hipStream_t)stream, hidden, ld_hidden, ctx,
                     Tmax, d, ctx_len, k, part, n_chunk);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_contrastive_finish(const float* part, int32_t n_chunk, const float* cand_p, int32_t B, int32_t k, float alpha,
                                     const mg_bf16* hidden, int64_t ld_hidden, int32_t d, mg_bf16* ctx, int32_t Tmax,
                                     int32_t* ctx_len, int32_t len_max, int32_t* src, const int64_t* token, int64_t* history,
                                     int64_t ld_history, int32_t history_cols, int64_t eos, int32_t* state, int32_t* d_pos, int32_t delta,
                                     int32_t pos_stride, void* stream) {
  const char* who = "mg_contrastive_finish";
  if (!part || !cand_p || !hidden || !ctx || !ctx_len || !src || !token || !state) MG_FAIL(MG_ERR_SHAPE, "%s: null pointer", who);
  if (B <= 0 || Tmax <= 0 || n_chunk != (Tmax + CS_CHUNK - 1) / CS_CHUNK)
    MG_FAIL(MG_ERR_SHAPE, "%s: need B, Tmax > 0 and n_chunk = ceil(Tmax / %d)", who, CS_CHUNK);
  if (len_max < 0 || len_max >= Tmax)
    MG_FAIL(MG_ERR_SHAPE, "%s: ctx_len reaches %d, no room to append in a store of Tmax = %d positions", who, len_max, Tmax);
  if (k < 1 || k > BK_MAX) MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= k <= %d, got %d", who, BK_MAX, k);
  if (!(alpha > 0.f && alpha <= 1.f)) MG_FAIL(MG_ERR_SHAPE, "%s: penalty_alpha must lie in (0, 1]", who);      // (NaN fails)
  if (d <= 0 || d % 256 != 0 || ld_hidden < d || ld_hidden % 8 != 0)
    MG_FAIL(MG_ERR_SHAPE, "%s: d must be a multiple of 256, ld_hidden >= d and a multiple of 8", who);
  if (pos_stride != 0 && pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "%s: pos_stride must be 0 or 1", who);
  if (history && (ld_history < history_cols || history_cols <= 0)) MG_FAIL(MG_ERR_SHAPE, "%s: bad history geometry", who);
  if (!MG_ALIGNED16(hidden) || !MG_ALIGNED16(ctx)) MG_FAIL(MG_ERR_ALIGN, "%s: hidden and ctx must be 16-byte aligned", who);
  if (((uintptr_t)part | (uintptr_t)cand_p | (uintptr_t)ctx_len | (uintptr_t)src | (uintptr_t)state | (uintptr_t)d_pos) & 3)
    MG_FAIL(MG_ERR_ALIGN, "%s: fp32 / int32 buffers must be 4-byte aligned", who);
  if (((uintptr_t)token | (uintptr_t)history) & 7) MG_FAIL(MG_ERR_ALIGN, "%s: token and history must be 8-byte aligned", who);
  ContrastFinishArgs a{part, n_chunk, cand_p, B, k, alpha, hidden, ld_hidden, d, ctx, Tmax, ctx_len, src, token, history,
                       ld_history, history ? history_cols : 0, eos, state, d_pos, pos_stride ? B * k : 1, delta};
  hipLaunchKernelGGL(contrastive_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  MG_CHECK_LAUNCH();
  return MG_OK;
}

extern "C" int mg_kv_broadcast_bf16(mg_bf16* kcache, mg_bf16* vcache, int32_t L, int32_t R, int32_t H, int32_t Smax, int32_t k,
                                    const int32_t* src, const int32_t* d_pos, int32_t pos_stride, int32_t pos_delta, void* stream) {
  const char* who = "mg_kv_broadcast_bf16";
  if (!kcache || !vcache || !src || !d_pos || L <= 0 || R <= 0 || H <= 0 || Smax <= 0) MG_FAIL(MG_ERR_SHAPE, "%s: bad arguments", who);
  if (k < 1 || k > BK_MAX || R % k != 0) MG_FAIL(MG_ERR_SHAPE, "%s: need 1 <= k <= %d dividing R = %d, got %d", who, BK_MAX, R, k);
  if (pos_stride != 0 && pos_stride != 1) MG_FAIL(MG_ERR_SHAPE, "%s: pos_stride must be 0 or 1", who);
  if (!MG_ALIGNED16(kcache) || !MG_ALIGNED16(vcache)) MG_FAIL(MG_ERR_ALIGN, "%s: the caches must be 16-byte aligned", who);
  if (((uintptr_t)src | (uintptr_t)d_pos) & 3) MG_FAIL(MG_ERR_ALIGN, "%s: src and d_pos must be 4-byte aligned", who);
  if (H > 65535 || L > 65535 || R > 65535) MG_FAIL(MG_ERR_SHAPE, "%s: grid too large", who);
  if (k == 1) return MG_OK;                   // a group of one row has no sibling
  hipLaunchKernelGGL(kv_broadcast_kernel, dim3(H, R, L), dim3(64), 0, (hipStream_t)stream, (uint4*)kcache, (uint4*)vcache, R, H, Smax,
                     k, src, d_pos, pos_stride, pos_delta);
  MG_CHECK_LAUNCH();
  return MG_OK;
}
