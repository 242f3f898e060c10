// d3pm_dedup.hip -- one denoiser row per distinct token of an utterance.
//
// The denoiser adds no positional term to the codec frames (ar_discrete.py:753: x = resps_emb[id], zeros on a padded frame), every
// later operation is local to a row or an attention whose query row sees its own q and the whole utterance's keys, so two frames of
// one utterance that carry the same id at the top of an iteration get the same logits, bit for bit.  Per iteration:
//   dedup_index_utt     one workgroup per utterance: class of a position = its id, or n_classes on a padded frame; the first canvas
//                       position of each class is its representative, ranked in position order; row_of (still local to the utterance),
//                       key_cls (the class of every position), the representatives' positions, the count
//   dedup_embed_rows    one wave per index r, which is both a compact row and a canvas position: the segments (an utterance owns its
//                       count rounded up to seg_align compact rows, back to back: seg_align = 1, the loop's, packs the rows densely --
//                       seg_len = cnt, seg_start = the exclusive prefix sum of the counts, m_live = their sum, no zero row inside a
//                       segment; 128 gives every utterance whole self-attention workgroups), the embedding row + moments + block-0 q
//                       of compact row r (a zero row with zero moments where a segment is padding, and from m_live up to the next
//                       multiple of 384, the least common multiple of the 192- and 128-row GEMM tiles), and row_of[r] made global
// No k | v row is copied into canvas order: the self-attention walks its keys through an index (attn32p_hd64 GATHER, d3pm_mfma_attn32.hip)
// -- in block 0 row key_cls[position] of the block-0 QKV table, in the later blocks row row_of[position] of the compact QKV rows.
// Nothing here reads anything back to the host: the counts stay in device memory and the GEMMs / attentions read them there.
#include <climits>

#include "d3pm_kernels.h"
#include "d3pm_fold_rows.h"

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

template <typename T>
__global__ __launch_bounds__(256) void dedup_embed_rows(const int32_t* __restrict__ tokens, const uint8_t* __restrict__ frame_mask, int mask_period,
                                                        int batch, int canvas, int n_classes, int d, int seg_align, const int32_t* __restrict__ cnt,
                                                        int32_t* __restrict__ seg_start, int32_t* __restrict__ seg_len, int32_t* __restrict__ m_live_out,
                                                        int32_t* __restrict__ row_of, const int32_t* __restrict__ rep_pos, int32_t* __restrict__ cid,
                                                        uint8_t* __restrict__ cmask, const T* __restrict__ table, T* __restrict__ x,
                                                        float* __restrict__ stats, bool quads, const T* __restrict__ qkv_table, T* __restrict__ q0,
                                                        T* __restrict__ zero0, T* __restrict__ zero1) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = batch * canvas;
  const int r = blockIdx.x * 4 + wave;      // wave-uniform
  if (r >= n) return;
  // the segments: every wave adds the padded counts up itself (`batch` uniform loads; nothing to wait for between launches)
  const int ub = r / canvas;
  int start = 0, u = -1, u_start = 0, u_cnt = 0, pos_start = 0, own_start = 0, own_len = 0;
  for (int b = 0; b < batch; ++b) {
    const int c = cnt[b], pad = (c + seg_align - 1) & ~(seg_align - 1);      // seg_align is 1 or 128 (dedup_index): a power of two
    if (r >= start && r < start + pad) { u = b; u_start = start; u_cnt = c; }
    if (b == ub) pos_start = start;
    if (b == r) { own_start = start; own_len = pad; }
    start += pad;
  }
  const int m_live = start, m_pad = (m_live + 383) / 384 * 384;      // <= n: the caller checks n % 384 == 0
  if (lane == 0) {
    if (r < batch) { seg_start[r] = own_start; seg_len[r] = own_len; }
    if (r == 0) *m_live_out = m_live;
  }
  // ---- canvas position r: global row_of
  if (lane == 0) row_of[r] += pos_start;
  // ---- compact row r
  if (r >= m_pad) return;      // (m_pad <= n also with seg_align = 128: a padded count never exceeds the canvas, a multiple of 128)
  int id = 0;
  bool live = false;
  if (u >= 0 && r - u_start < u_cnt) {
    const size_t row = static_cast<size_t>(u) * canvas + rep_pos[static_cast<size_t>(u) * canvas + (r - u_start)];
    id = clamp_id(tokens[row], n_classes);
    live = frame_mask[row % mask_period] != 0;
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
  const int n = a.batch * a.canvas;
  const size_t lds = (2 * static_cast<size_t>(a.n_classes + 1) + 4) * sizeof(int);
  dedup_index_utt<<<dim3(a.batch), dim3(256), lds, s>>>(a.tokens, a.frame_mask, a.mask_period, a.canvas, a.n_classes, ix.cnt, ix.row_of, ix.rep_pos, ix.key_cls);
  D3PM_LAUNCH_CHECK();
  const dim3 grid(static_cast<unsigned>((n + 3) / 4)), block(256);
  auto go = [&](auto* tag) {
    using U = std::remove_pointer_t<decltype(tag)>;
    dedup_embed_rows<U><<<grid, block, 0, s>>>(a.tokens, a.frame_mask, a.mask_period, a.batch, a.canvas, a.n_classes, a.d, a.seg_align, ix.cnt, ix.seg_start,
                                               ix.seg_len, ix.m_live, ix.row_of, ix.rep_pos, ix.cid, ix.cmask, static_cast<const U*>(a.table), static_cast<U*>(a.x),
                                               a.stats, a.quads, static_cast<const U*>(a.qkv_table), static_cast<U*>(a.q0),
                                               static_cast<U*>(a.zero[0]), static_cast<U*>(a.zero[1]));
  };
  if (dtype == D3PM_F16) go(static_cast<f16*>(nullptr)); else go(static_cast<bf16*>(nullptr));
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // namespace d3pm
