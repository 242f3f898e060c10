// d3pm_dedup.hip -- one denoiser row per distinct token of an utterance.
//
// The denoiser adds no positional term to the codec frames (ar_discrete.py:753: x = resps_emb[id], zeros on a padded frame), every
// later operation is local to a row or an attention whose query row sees its own q and the whole utterance's keys, so two frames of
// one utterance that carry the same id at the top of an iteration get the same logits, bit for bit.  Per iteration:
//   dedup_index_utt     one workgroup per utterance: class of a position = its id, or n_classes on a padded frame; the first canvas
//                       position of each class is its representative, ranked in position order; row_of (still local to the utterance),
//                       key_cls (the class of every position), the representatives' positions, the count
//   dedup_embed_rows    a fixed grid (4 workgroups per CU) whose waves stride over the canvas positions and over the compact rows
//                       below m_pad; every workgroup scans the counts once for the segments (an utterance owns its
//                       count rounded up to seg_align compact rows, back to back: seg_align = 1, the loop's, packs the rows densely --
//                       seg_len = cnt, seg_start = the exclusive prefix sum of the counts, m_live = their sum, no zero row inside a
//                       segment; 128 gives every utterance whole self-attention workgroups), the embedding row + moments + block-0 q
//                       of compact row r (a zero row with zero moments where a segment is padding, and from m_live up to the next
//                       multiple of 384, the least common multiple of the 192- and 128-row GEMM tiles), and row_of[r] of canvas
//                       position r made global
// No k | v row is copied into canvas order: the self-attention walks its keys through an index (attn32p_hd64 GATHER, d3pm_mfma_attn32.hip)
// -- in block 0 row key_cls[position] of the block-0 QKV table, in the later blocks row row_of[position] of the compact QKV rows.
// Nothing here reads anything back to the host: the counts stay in device memory and the GEMMs / attentions read them there.
#include <climits>

#include "d3pm_kernels.h"
#include "d3pm_fold_rows.h"
#include "d3pm_plan.h"

namespace d3pm {
namespace {

__device__ __forceinline__ int clamp_id(int id, int n_classes) { return id < 0 ? 0 : (id >= n_classes ? n_classes - 1 : id); }

__global__ __launch_bounds__(256) void dedup_index_utt(const int32_t* __restrict__ tokens, const uint8_t* __restrict__ frame_mask, int mask_period,
                                                       int canvas, int n_classes, int32_t* __restrict__ cnt, int32_t* __restrict__ row_of,
                                                       int32_t* __restrict__ rep_pos, int32_t* __restrict__ key_cls) {
  extern __shared__ int dedup_sm[];
  int* first = dedup_sm;                      // [n_classes + 1] first position of a class
  int* rank = first + n_classes + 1;          // [n_classes + 1] rank of its representative
  int* wsum = rank + n_classes + 1;           // [4]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = static_cast<size_t>(b) * canvas;
  for (int c = tid; c <= n_classes; c += 256) first[c] = INT_MAX;
  __syncthreads();
  auto class_of = [&](int j) {
    const size_t r = row0 + j;
    return frame_mask[r % mask_period] ? clamp_id(tokens[r], n_classes) : n_classes;
  };
  for (int j = tid; j < canvas; j += 256) atomicMin(&first[class_of(j)], j);
  __syncthreads();
  int base = 0;
  for (int j0 = 0; j0 < canvas; j0 += 256) {      // block-uniform trip count
    const int j = j0 + tid;
    int c = 0;
    bool rep = false;
    if (j < canvas) { c = class_of(j); rep = first[c] == j; }
    const unsigned long long m = __ballot(rep);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (rep) {
      const int k = off + __popcll(m & ((1ull << lane) - 1ull));
      rank[c] = k;
      rep_pos[row0 + k] = j;
    }
    base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  for (int j = tid; j < canvas; j += 256) {
    const int c = class_of(j);
    row_of[row0 + j] = rank[c];
    if (key_cls) key_cls[row0 + j] = c;      // kernel-uniform
  }
  if (tid == 0) cnt[b] = base;
}

// A fixed grid of kEmbedGrid workgroups, whatever batch * canvas is (one wave per index used to be 6144 nearly empty workgroups at the
// benchmark's 24 576 rows: a launch bound by its dispatch, 23 us at 64 live rows).  Every workgroup forms the segment prefix once, in
// LDS, and its waves then stride over (1) the canvas positions, 64 per wave and trip, and (2) the compact rows below m_pad, one wave
// per row and trip -- m_pad comes out of the prefix, on the device, so no wave is launched for a row nobody owns.
// The prefix bounds the batch (kDedupMaxBatch, d3pm_kernels.h: refused with D3PM_E_SHAPE above it; the sampler loop keeps every row there).
constexpr int kEmbedGrid = 4 * kCUs;

template <typename T>
__global__ __launch_bounds__(256) void dedup_embed_rows(const int32_t* __restrict__ tokens, const uint8_t* __restrict__ frame_mask, int mask_period,
                                                        int batch, int canvas, int n_classes, int d, int seg_align, const int32_t* __restrict__ cnt,
                                                        int32_t* __restrict__ seg_start, int32_t* __restrict__ seg_len, int32_t* __restrict__ m_live_out,
                                                        int32_t* __restrict__ row_of, const int32_t* __restrict__ rep_pos, int32_t* __restrict__ cid,
                                                        uint8_t* __restrict__ cmask, const T* __restrict__ table, T* __restrict__ x,
                                                        float* __restrict__ stats, bool quads, const T* __restrict__ qkv_table, T* __restrict__ q0,
                                                        T* __restrict__ zero0, T* __restrict__ zero1) {
  extern __shared__ int embed_sm[];
  int* start = embed_sm;              // [batch + 1] exclusive prefix of the padded counts; start[batch] = m_live
  int* wsum = start + batch + 1;      // [4]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = batch * canvas;
  // ---- the segments: one scan per workgroup (256 utterances per trip; the trip count is block-uniform)
  int base = 0;
  for (int b0 = 0; b0 < batch; b0 += 256) {
    const int b = b0 + tid;
    const int pad = b < batch ? (cnt[b] + seg_align - 1) & ~(seg_align - 1) : 0;      // seg_align is 1 or 128 (dedup_index): a power of two
    int v = pad;                                                                      // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int o = __shfl_up(v, off, kWave);
      if (lane >= off) v += o;
    }
    if (lane == kWave - 1) wsum[wave] = v;
    __syncthreads();
    int before = base;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (b < batch) start[b] = before + v - pad;
    base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (tid == 0) start[batch] = base;
  __syncthreads();
  const int m_live = base, m_pad = (m_live + 383) / 384 * 384;      // <= n: the caller checks n % 384 == 0
  if (blockIdx.x == 0) {
    for (int b = tid; b < batch; b += 256) { seg_start[b] = start[b]; seg_len[b] = start[b + 1] - start[b]; }
    if (tid == 0) *m_live_out = m_live;
  }
  const int gw = blockIdx.x * 4 + wave, waves = gridDim.x * 4;      // wave-uniform
  // ---- canvas positions: global row_of
  for (int r0 = gw * kWave; r0 < n; r0 += waves * kWave) {
    const int r = r0 + lane;
    if (r < n) row_of[r] += start[r / canvas];
  }
  // ---- compact rows (m_pad <= n also with seg_align = 128: a padded count never exceeds the canvas, a multiple of 128)
  const int m_end = m_pad < n ? m_pad : n;      // (never the second with counts dedup_index_utt wrote; no store leaves the arrays with any others)
  for (int r = gw; r < m_end; r += waves) {
    int id = 0;
    bool live = false;
    if (r < m_live) {
      int lo = 0, hi = batch - 1;      // the last utterance whose segment starts at or below r: the one that owns r (empty segments share a start)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= r) lo = mid; else hi = mid - 1;
      }
      const int u = lo, k = r - start[u];
      if (k < cnt[u]) {
        const size_t row = static_cast<size_t>(u) * canvas + rep_pos[static_cast<size_t>(u) * canvas + k];
        id = clamp_id(tokens[row], n_classes);
        live = frame_mask[row % mask_period] != 0;
      }
    }
    if (table) embed_row_stats<T>(table, id, live, x, r, d, n_classes, stats, quads, lane);      // a zero row with zero moments unless live
    if (qkv_table) {
      const Vec8<T>* ts = reinterpret_cast<const Vec8<T>*>(qkv_table + static_cast<size_t>(live ? id : n_classes) * 3 * d);
      Vec8<T>* tq = reinterpret_cast<Vec8<T>*>(q0 + static_cast<size_t>(r) * d);
      for (int c = lane; c < (d >> 3); c += kWave) tq[c] = ts[c];
    }
    if (lane == 0) {
      cid[r] = live ? id : n_classes;
      cmask[r] = live ? 1 : 0;
    }
    if (r >= m_live) {
      if (zero0) { Vec8<T>* z = reinterpret_cast<Vec8<T>*>(zero0 + static_cast<size_t>(r) * d); for (int c = lane; c < (d >> 3); c += kWave) z[c] = Vec8<T>{}; }
      if (zero1) { Vec8<T>* z = reinterpret_cast<Vec8<T>*>(zero1 + static_cast<size_t>(r) * d); for (int c = lane; c < (d >> 3); c += kWave) z[c] = Vec8<T>{}; }
    }
  }
}

}  // namespace

int dedup_index(int dtype, const DedupArgs& a, hipStream_t s) {
  const DedupIndex& ix = a.ix;
  D3PM_REQUIRE(a.tokens && a.frame_mask && a.mask_period > 0 && a.batch > 0 && a.canvas > 0 && a.n_classes > 0 && ix.cnt && ix.seg_start && ix.seg_len &&
                   ix.m_live && ix.row_of && ix.rep_pos && ix.cid && ix.cmask,
               D3PM_E_ARG, "row deduplication: null pointer");
  D3PM_REQUIRE(a.seg_align == 1 || a.seg_align == 128, D3PM_E_ARG, "row deduplication: seg_align is 1 or 128, not %d", a.seg_align);
  // (canvas a multiple of 128: a segment never exceeds its utterance's canvas at either alignment, so the compact rows fit the capacity)
  D3PM_REQUIRE(a.n_classes <= kDedupMaxClasses && a.canvas % 128 == 0 && (static_cast<long long>(a.batch) * a.canvas) % 384 == 0, D3PM_E_SHAPE,
               "row deduplication: at most %d classes, canvas a multiple of 128 and batch * canvas a multiple of 384", kDedupMaxClasses);
  D3PM_REQUIRE((dtype == D3PM_F16 || dtype == D3PM_BF16) && a.d % 8 == 0 && (!a.quads || a.d == 512) && (!a.table || (a.x && a.stats)) &&
                   (a.qkv_table != nullptr) == (a.q0 != nullptr),
               D3PM_E_ARG, "row deduplication: bad embedding arguments");
  D3PM_REQUIRE(a.batch <= kDedupMaxBatch, D3PM_E_SHAPE, "row deduplication: at most %d utterances", kDedupMaxBatch);
  const size_t lds = (2 * static_cast<size_t>(a.n_classes + 1) + 4) * sizeof(int);
  dedup_index_utt<<<dim3(a.batch), dim3(256), lds, s>>>(a.tokens, a.frame_mask, a.mask_period, a.canvas, a.n_classes, ix.cnt, ix.row_of, ix.rep_pos, ix.key_cls);
  D3PM_LAUNCH_CHECK();
  const dim3 grid(kEmbedGrid), block(256);
  const size_t embed_lds = (static_cast<size_t>(a.batch) + 1 + 4) * sizeof(int);
  auto go = [&](auto* tag) {
    using U = std::remove_pointer_t<decltype(tag)>;
    dedup_embed_rows<U><<<grid, block, embed_lds, s>>>(a.tokens, a.frame_mask, a.mask_period, a.batch, a.canvas, a.n_classes, a.d, a.seg_align, ix.cnt, ix.seg_start,
                                               ix.seg_len, ix.m_live, ix.row_of, ix.rep_pos, ix.cid, ix.cmask, static_cast<const U*>(a.table), static_cast<U*>(a.x),
                                               a.stats, a.quads, static_cast<const U*>(a.qkv_table), static_cast<U*>(a.q0),
                                               static_cast<U*>(a.zero[0]), static_cast<U*>(a.zero[1]));
  };
  if (dtype == D3PM_F16) go(static_cast<f16*>(nullptr)); else go(static_cast<bf16*>(nullptr));
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // namespace d3pm
