// d3pm_nar_train.hip -- backward-pass kernels of the stock NAR model's training step that d3pm_train.hip does not already have.
//
// The reference trains the NAR stage with autograd over NAR.forward's training branch (the reference's vall_e/vall_e/nar.py:53-74:
// one quantizer level l_b per utterance, levels 0 .. l_b of the response in, level l_b + 1 the target) and Base.forward
// (base.py:403-488: input assembly :427-435, AdaLN blocks :136-234, classifier :440, cross-entropy over the response rows :445-488).
// The matrix products, the attention, the GELU and the row masks of that backward pass are the entries of d3pm_train.hip; here are
// the three pieces that are the NAR's own (include/d3pm_hip.h, "NAR training step"; host side vall_e/vall_e/nar_train.py):
//   adaln_bwd_rows / adaln_bwd_cols   AdaLN.forward base.py:145-158 backward, with `(k h).detach()` (:154) a constant
//   nar_embed_bwd_rows                the scatter-add behind nar_embed_rows (d3pm_nar.hip; base.py:427-435, MultiEmbedding :244-274)
//   nar_ce_rows                       F.cross_entropy(..., ignore_index) of base.py:482-488 per grid row, and its gradient
// fp32 throughout, fp32 accumulation.  The sums across rows -- (dlog_gamma | dbeta) of AdaLN and the table rows that several tokens
// share -- have ONE writer per destination that adds its contributions in row order: no atomics, so the gradients are the same bits
// from run to run and a row that must not contribute (masked, behind an utterance's total) provably changes none of them.
#include <cmath>

#include "d3pm_kernels.h"

namespace d3pm {
namespace {

constexpr float kAdaEps = 1e-5f, kAdaK = 0.1f, kAdaC = 2.0f;      // AdaLN(eps=1e-5, k=0.1, c=2), base.py:137

// mean and 1 / sqrt(var + eps) of one row by one wave, as adaln_rows<float> computes them (so h has the forward's bits)
__device__ __forceinline__ void row_moments(const float* __restrict__ xr, int d, int lane, float& mean, float& rstd) {
  float s = 0.f;
  for (int c = lane; c < d; c += kWave) s += xr[c];
  mean = wave_sum(s) / static_cast<float>(d);
  float q = 0.f;
  for (int c = lane; c < d; c += kWave) {
    const float t = xr[c] - mean;
    q += t * t;
  }
  rstd = rsqrtf(wave_sum(q) / static_cast<float>(d) + kAdaEps);
}

// One wave per row.  y = exp(lg) * (f h) + beta with h = LayerNorm(x) and f = c (1 - k h) a CONSTANT of the backward pass (the
// detach):  dh = dy exp(lg) f;  dx (+)= rstd (dh - mean(dh) - h mean(dh h)).  A masked row is not read; its dx row is zeroed, or
// left alone when accumulating.
__global__ __launch_bounds__(256) void adaln_bwd_rows(const float* __restrict__ x, const float* __restrict__ dy,
                                                      const float* __restrict__ emb_row, const uint8_t* __restrict__ row_mask, int M,
                                                      int d, float* dx, int accumulate) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= M) return;
  float* dxr = dx + static_cast<size_t>(row) * d;
  if (!row_mask[row]) {
    if (!accumulate)
      for (int c = lane; c < d; c += kWave) dxr[c] = 0.f;
    return;
  }
  const float* xr = x + static_cast<size_t>(row) * d;
  const float* gr = dy + static_cast<size_t>(row) * d;
  float mean, rstd;
  row_moments(xr, d, lane, mean, rstd);
  float sg = 0.f, sgh = 0.f;
  for (int c = lane; c < d; c += kWave) {
    const float h = (xr[c] - mean) * rstd;
    const float dh = gr[c] * expf(emb_row[c]) * (kAdaC * (1.0f - kAdaK * h));
    sg += dh;
    sgh += dh * h;
  }
  const float mg = wave_sum(sg) / static_cast<float>(d), mgh = wave_sum(sgh) / static_cast<float>(d);
  for (int c = lane; c < d; c += kWave) {
    const float h = (xr[c] - mean) * rstd;
    const float dh = gr[c] * expf(emb_row[c]) * (kAdaC * (1.0f - kAdaK * h));
    const float v = rstd * (dh - mg - h * mgh);
    dxr[c] = accumulate ? dxr[c] + v : v;
  }
}

// dlg[c] += sum_rows dy exp(lg) f h,  dbeta[c] += sum_rows dy  over the unmasked rows.  One workgroup owns kColTile columns and walks
// ALL rows: wave w takes rows w, w + 8, ... in order (row moments recomputed: two passes over a row that the caches hold), a lane
// keeps its four columns' partial sums in registers; the eight waves' partials meet in LDS and are added in wave order to the one
// demb_row element this workgroup alone writes.
constexpr int kColTile = 256, kColWaves = 8;
__global__ __launch_bounds__(kColWaves * 64) void adaln_bwd_cols(const float* __restrict__ x, const float* __restrict__ dy,
                                                                  const float* __restrict__ emb_row,
                                                                  const uint8_t* __restrict__ row_mask, int M, int d, float* demb_row) {
  __shared__ float part[kColWaves][2][kColTile];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c0 = blockIdx.x * kColTile;
  float alg[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f}, g[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + lane + 64 * k;
    g[k] = c < d ? expf(emb_row[c]) : 0.f;
  }
  for (int row = wave; row < M; row += kColWaves) {
    if (!row_mask[row]) continue;      // wave-uniform
    const float* xr = x + static_cast<size_t>(row) * d;
    const float* gr = dy + static_cast<size_t>(row) * d;
    float mean, rstd;
    row_moments(xr, d, lane, mean, rstd);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + lane + 64 * k;
      if (c < d) {
        const float h = (xr[c] - mean) * rstd;
        const float dh = gr[c] * g[k] * (kAdaC * (1.0f - kAdaK * h));
        alg[k] += dh * h;
        ab[k] += gr[c];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    part[wave][0][lane + 64 * k] = alg[k];
    part[wave][1][lane + 64 * k] = ab[k];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * kColTile; e += kColWaves * 64) {
    const int which = e / kColTile, cc = e % kColTile, c = c0 + cc;
    if (c >= d) continue;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < kColWaves; ++w) s += part[w][which][cc];
    demb_row[which * d + c] += s;
  }
}

// The table rows of one "job" -- the text table, prompt level l, response level l -- collide wherever a token repeats, inside an
// utterance or across the batch.  Workgroup (grid row, level) looks up its own token; if an earlier row of the job carries the same
// token it leaves, otherwise it is that token's owner: it adds the dx rows of every row of the job with this token, in row order, and
// is the only writer of the table row.  The 2 * batch separator rows are summed by the workgroup of the first one.
// Rows at or past an utterance's total (or outside the grid) are never read; an id outside [0, n_tokens) has no table row and adds
// nowhere (the forward clamps it; such an id is outside the contract); an absent prompt level (-1) is such an id.
struct NarJobs {
  const int32_t *lens, *text, *prom, *resp;
  int tt_max, tp_max, n_prom_levels, tr_max, resp_stride, t_max;
  // kind 0 text, 1 prompt, 2 response: first grid position and row count of utterance b's segment, cut at the index array and the grid
  __device__ int offset(int kind, int b) const { return kind == 0 ? 0 : (kind == 1 ? lens[b * 3] + 1 : lens[b * 3] + lens[b * 3 + 1] + 2); }
  __device__ int count(int kind, int b) const {
    const int n = min(lens[b * 3 + kind], kind == 0 ? tt_max : (kind == 1 ? tp_max : tr_max));
    return max(0, min(n, t_max - offset(kind, b)));
  }
  __device__ int id(int kind, int level, int b, int f) const {
    return kind == 0 ? text[b * tt_max + f]
                     : (kind == 1 ? prom[(static_cast<size_t>(b) * tp_max + f) * n_prom_levels + level]
                                  : resp[(static_cast<size_t>(b) * tr_max + f) * resp_stride + level]);
  }
};

__global__ void nar_embed_bwd_rows(NarJobs j, int n_given, const float* __restrict__ dx, float* d_text, float* d_prom, float* d_resp,
                                   float* d_sep, int batch, int d, int n_tokens) {
  const int row = blockIdx.x, level = blockIdx.y, b = row / j.t_max, pos = row % j.t_max;
  const int tt = j.lens[b * 3], tp = j.lens[b * 3 + 1], tr = j.lens[b * 3 + 2];
  if (pos >= tt + tp + tr + 2) return;
  if (pos == tt || pos == tt + 1 + tp) {      // separators: one owner for the whole batch
    if (level != 0 || b != 0 || pos != tt) return;
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
      float acc = 0.f;
      for (int u = 0; u < batch; ++u) {
        const int p0 = j.lens[u * 3], p1 = p0 + 1 + j.lens[u * 3 + 1];
        if (p0 >= 0 && p0 < j.t_max) acc += dx[(static_cast<size_t>(u) * j.t_max + p0) * d + c];
        if (p1 >= 0 && p1 < j.t_max) acc += dx[(static_cast<size_t>(u) * j.t_max + p1) * d + c];
      }
      d_sep[c] += acc;
    }
    return;
  }
  const int kind = pos < tt ? 0 : (pos < tt + 1 + tp ? 1 : 2);
  if (level >= (kind == 0 ? 1 : (kind == 1 ? j.n_prom_levels : n_given))) return;
  const int f = pos - j.offset(kind, b);
  if (f >= j.count(kind, b)) return;          // behind the index array: the forward's caller keeps lens inside it
  const int own = j.id(kind, level, b, f);
  if (own < 0 || own >= n_tokens) return;
  // everything above is uniform over the workgroup
  int earlier = 0;
  for (int u = 0; u <= b; ++u) {
    const int n = u < b ? j.count(kind, u) : f;
    for (int g = threadIdx.x; g < n; g += blockDim.x) earlier |= j.id(kind, level, u, g) == own;
  }
  if (__syncthreads_or(earlier)) return;
  float* table = kind == 0 ? d_text : (kind == 1 ? d_prom : d_resp) + static_cast<size_t>(level) * n_tokens * d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) {
    float acc = 0.f;
    for (int u = b; u < batch; ++u) {
      const int n = j.count(kind, u), off = j.offset(kind, u);
      for (int g = u == b ? f : 0; g < n; ++g)
        if (j.id(kind, level, u, g) == own) acc += dx[(static_cast<size_t>(u) * j.t_max + off + g) * d + c];
    }
    table[static_cast<size_t>(own) * d + c] += acc;
  }
}

// One wave per grid row.  Response frame f of utterance b sits in grid row t_text + t_prompt + 2 + f and is scored against
// resp[b][f][levels[b] + 1]:  row_loss = logsumexp(logits) - logits[target],  dlogits = (softmax(logits) - onehot(target)) gscale.
// Every other row (text, separators, prompt, padding) gets row_loss 0 and a zero dlogits row: upstream's ignore_index.
__global__ __launch_bounds__(256) void nar_ce_rows(const float* __restrict__ logits, int ldl, const int32_t* __restrict__ lens,
                                                   const int32_t* __restrict__ resp, int tr_max, int resp_stride,
                                                   const int32_t* __restrict__ levels, int batch, int t_max, int K, float gscale,
                                                   float* __restrict__ row_loss, float* __restrict__ dlogits, int ldd) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= batch * t_max) return;
  const int b = row / t_max, pos = row % t_max;
  const int tt = lens[b * 3], tp = lens[b * 3 + 1], tr = lens[b * 3 + 2];
  const int f = pos - (tt + tp + 2);
  float* dr = dlogits ? dlogits + static_cast<size_t>(row) * ldd : nullptr;
  if (f < 0 || f >= tr || f >= tr_max) {
    if (lane == 0) row_loss[row] = 0.f;
    if (dr)
      for (int j = lane; j < K; j += kWave) dr[j] = 0.f;
    return;
  }
  int col = levels[b] + 1;
  col = col < 0 ? 0 : (col >= resp_stride ? resp_stride - 1 : col);
  int tg = resp[(static_cast<size_t>(b) * tr_max + f) * resp_stride + col];
  tg = tg < 0 ? 0 : (tg >= K ? K - 1 : tg);
  const float* lr = logits + static_cast<size_t>(row) * ldl;
  float mx = -INFINITY;
  for (int j = lane; j < K; j += kWave) mx = fmaxf(mx, lr[j]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < K; j += kWave) sum += expf(lr[j] - mx);
  sum = wave_sum(sum);
  if (lane == 0) row_loss[row] = (mx + logf(sum)) - lr[tg];
  if (dr)
    for (int j = lane; j < K; j += kWave) dr[j] = (expf(lr[j] - mx) / sum - (j == tg ? 1.f : 0.f)) * gscale;
}

}  // namespace
}  // namespace d3pm

using namespace d3pm;

extern "C" {

int d3pm_op_adaln_bwd_f32(const float* x, const float* dy, const float* emb_row, const uint8_t* row_mask, int M, int d, float* dx,
                          int accumulate, float* demb_row, void* stream) {
  D3PM_REQUIRE(x && dy && emb_row && row_mask && dx && demb_row, D3PM_E_ARG, "d3pm_op_adaln_bwd_f32: null pointer");
  D3PM_REQUIRE(M > 0 && d > 0, D3PM_E_ARG, "d3pm_op_adaln_bwd_f32: M = %d and d = %d must be positive", M, d);
  hipStream_t s = static_cast<hipStream_t>(stream);
  adaln_bwd_rows<<<(M + 3) / 4, 256, 0, s>>>(x, dy, emb_row, row_mask, M, d, dx, accumulate);
  adaln_bwd_cols<<<(d + kColTile - 1) / kColTile, kColWaves * 64, 0, s>>>(x, dy, emb_row, row_mask, M, d, demb_row);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int d3pm_op_nar_embed_bwd_f32(const int32_t* lens, const int32_t* text, int tt_max, const int32_t* prom, int tp_max, int n_prom_levels,
                              const int32_t* resp, int tr_max, int resp_stride, int n_given, const float* dx, float* d_text,
                              float* d_prom, float* d_resp, float* d_sep, int batch, int t_max, int d, int n_tokens, void* stream) {
  D3PM_REQUIRE(lens && text && prom && resp && dx && d_text && d_prom && d_resp && d_sep, D3PM_E_ARG,
               "d3pm_op_nar_embed_bwd_f32: null pointer");
  D3PM_REQUIRE(batch > 0 && t_max > 0 && tt_max > 0 && tp_max > 0 && tr_max > 0 && d > 0 && n_tokens > 0 && n_prom_levels > 0 &&
                   n_given >= 1 && n_given <= resp_stride,
               D3PM_E_ARG, "d3pm_op_nar_embed_bwd_f32: sizes must be positive and 1 <= n_given <= resp_stride");
  const int levels = n_prom_levels > n_given ? n_prom_levels : n_given;
  D3PM_REQUIRE(static_cast<long>(batch) * t_max <= 0x7fffffffL && levels <= 65535, D3PM_E_SHAPE,
               "d3pm_op_nar_embed_bwd_f32: %d x %d rows x %d levels exceed the grid", batch, t_max, levels);
  NarJobs j{lens, text, prom, resp, tt_max, tp_max, n_prom_levels, tr_max, resp_stride, t_max};
  nar_embed_bwd_rows<<<dim3(batch * t_max, levels), d >= 256 ? 256 : 64, 0, static_cast<hipStream_t>(stream)>>>(
      j, n_given, dx, d_text, d_prom, d_resp, d_sep, batch, d, n_tokens);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int d3pm_op_nar_ce_f32(const float* logits, int ldl, const int32_t* lens, const int32_t* resp, int tr_max, int resp_stride,
                       const int32_t* levels, int batch, int t_max, int n_tokens, float gscale, float* row_loss, float* dlogits, int ldd,
                       void* stream) {
  D3PM_REQUIRE(logits && lens && resp && levels && row_loss, D3PM_E_ARG, "d3pm_op_nar_ce_f32: null pointer");
  D3PM_REQUIRE(batch > 0 && t_max > 0 && tr_max > 0 && resp_stride > 1 && n_tokens > 1 && ldl >= n_tokens && (!dlogits || ldd >= n_tokens),
               D3PM_E_ARG, "d3pm_op_nar_ce_f32: sizes must be positive, resp_stride and n_tokens above 1, ldl / ldd >= n_tokens");
  D3PM_REQUIRE(static_cast<long>(batch) * t_max <= 0x7fffffffL, D3PM_E_SHAPE, "d3pm_op_nar_ce_f32: %d x %d rows exceed the grid", batch, t_max);
  const int rows = batch * t_max;
  nar_ce_rows<<<(rows + 3) / 4, 256, 0, static_cast<hipStream_t>(stream)>>>(logits, ldl, lens, resp, tr_max, resp_stride, levels, batch,
                                                                            t_max, n_tokens, gscale, row_loss, dlogits, ldd);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // extern "C"
