// C ABI (include/smaml.h) and the host-side driver of the STGCN-LSTM MAML hot path.
//
// The inner loop (train_hybrid_maml_v5.py:110-141) and the meta-step
// (train_hybrid_maml_v5.py:144-184) run here in C++: Python calls one entry point per
// meta-step and never sees an inner step. Everything for all tasks of the meta-batch
// is batched into each launch (blockIdx.z = task, per-task fast weights).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <dlfcn.h>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "devbuf.h"
#include "kernels.h"
#include "smaml.h"

using namespace smaml;
using HipBuf = DevBuf<HipAlloc>;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(x)                                                                              \
  do {                                                                                          \
    hipError_t e_ = (x);                                                                        \
    if (e_ != hipSuccess) return fail(SMAML_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define TRY(x)                \
  do {                        \
    int r_ = (x);             \
    if (r_ != SMAML_OK) return r_; \
  } while (0)

constexpr int64_t PAD = 64;  // floats: every tensor offset is 256-B aligned

int64_t pad_up(int64_t x) { return (x + PAD - 1) / PAD * PAD; }

struct Spec {
  int64_t off, size;
};

int check_dims(const smaml_dims* d) {
  if (!d) return fail(SMAML_EINVAL, "dims is NULL");
  if (d->num_nodes <= 0 || d->window_size <= 0 || d->lstm_num_layers <= 0 ||
      d->lstm_num_layers > MAX_LAYERS || d->forecast_horizon <= 0 || d->output_channels <= 0)
    return fail(SMAML_EINVAL, "non-positive dimension");
  if (d->input_channels % 4 || d->hidden_channels % 4)
    return fail(SMAML_EINVAL, "input/hidden channels must be multiples of 4");
  if (d->lstm_hidden_size != 32 && d->lstm_hidden_size != 64 && d->lstm_hidden_size != 128 &&
      d->lstm_hidden_size != 256)
    return fail(SMAML_EINVAL, "lstm_hidden_size must be 32, 64, 128 or 256");
  if (d->forecast_horizon * d->output_channels > 128)
    return fail(SMAML_EINVAL, "forecast_horizon*output_channels must be <= 128");
  if (d->output_channels > d->input_channels)
    return fail(SMAML_EINVAL, "output_channels must not exceed input_channels (targets come from inputs)");
  return SMAML_OK;
}

// What the LSTM gate-GEMM, BPTT and head launches need beyond check_dims (a context that only runs the GCN
// entry points, e.g. the GCNConv drop-in's hidden_channels = 4, needs none of it). Called by every entry
// point that plans such a launch, before it allocates or launches anything.
//  - hidden_channels % 16: the tile loaders of the default path (loaders.h "tile loaders": SegKCt,
//    SegGateBt, SegGateImg, k_xg_dedup, the batch-1 k_gemm_nt, the 4-segment tangent loaders) pick a
//    segment once per BK = 16 wide K tile, and the gate images hold w / 16 tiles per segment: a layer-0
//    input segment that is no multiple of 16 would read across row ends and past the operand.
//  - forecast_horizon*output_channels % 4: dpred / pred rows are read 16 bytes at a time (k_gemm_nn's
//    RowMajorKC, the head weight gradients); a row that is no multiple of 4 floats misaligns every other
//    row and the K tail reads past the row (at the last row, past the buffer).
int check_lstm_dims(const smaml_dims& d, const char* who) {
  if (d.hidden_channels % 16)
    return fail(SMAML_EINVAL, std::string(who) + ": hidden_channels must be a multiple of 16 for the LSTM and head "
                                  "entry points (the layer-0 K segment of the gate GEMM tiles), got " +
                                  std::to_string(d.hidden_channels));
  if ((d.forecast_horizon * d.output_channels) % 4)
    return fail(SMAML_EINVAL, std::string(who) + ": forecast_horizon*output_channels must be a multiple of 4 for "
                                  "the LSTM and head entry points (16-byte reads of prediction rows), got " +
                                  std::to_string(d.forecast_horizon * d.output_channels));
  return SMAML_OK;
}

void layout(const smaml_dims& d, int which, std::vector<Spec>& specs, int64_t& total) {
  specs.clear();
  int64_t off = 0;
  auto add = [&](int64_t n) {
    specs.push_back({off, n});
    off = pad_up(off + n);
  };
  const int64_t H = d.lstm_hidden_size, G = 4 * H;
  if (which == 0) {
    for (int l = 0; l < d.lstm_num_layers; ++l) {
      const int64_t cin = l == 0 ? d.hidden_channels : H;
      add(G * cin);  // weight_ih_l
      add(G * H);    // weight_hh_l
      add(G);        // bias_ih_l
      add(G);        // bias_hh_l
    }
    add((int64_t)d.forecast_horizon * d.output_channels * H);  // output_layer.weight
    add((int64_t)d.forecast_horizon * d.output_channels);      // output_layer.bias
  } else {
    int64_t cin = d.input_channels;
    for (int k = 0; k < 4; ++k) {
      add(d.hidden_channels);        // convK.bias
      add(d.hidden_channels * cin);  // convK.lin.weight
      cin = d.hidden_channels;
    }
  }
  total = off;
}

int build_ell(const int64_t* ei, int64_t E, int N, std::vector<int32_t>& cols, std::vector<float>& vals) {
  cols.assign((size_t)N * ELLW, 0);
  vals.assign((size_t)N * ELLW, 0.f);
  std::vector<float> deg(N, 1.f);  // self loop (add_remaining_self_loops, fill 1)
  const int64_t* src = ei;
  const int64_t* dst = ei + E;
  for (int64_t e = 0; e < E; ++e) {
    if (src[e] < 0 || src[e] >= N || dst[e] < 0 || dst[e] >= N)
      return fail(SMAML_EINVAL, "edge_index references a node outside [0, num_nodes)");
    if (src[e] != dst[e]) deg[dst[e]] += 1.f;
  }
  std::vector<float> dinv(N);
  for (int i = 0; i < N; ++i) dinv[i] = 1.f / std::sqrt(deg[i]);
  std::vector<int> fill(N, 0);
  for (int64_t e = 0; e < E; ++e) {
    const int64_t s = src[e], t = dst[e];
    if (s == t) continue;
    if (fill[t] >= ELLW - 1) return fail(SMAML_EINVAL, "node in-degree exceeds the ELL width (7)");
    cols[(size_t)t * ELLW + fill[t]] = (int32_t)s;
    vals[(size_t)t * ELLW + fill[t]] = dinv[s] * dinv[t];
    ++fill[t];
  }
  for (int i = 0; i < N; ++i) {
    for (int j = fill[i]; j < ELLW; ++j) cols[(size_t)i * ELLW + j] = i;
    vals[(size_t)i * ELLW + fill[i]] = dinv[i] * dinv[i];
  }
  return SMAML_OK;
}

// A_hat as CSR for any in-degree and optional edge weights (smaml.h: smaml_graph_csr states the rules; PyG 2.x
// gcn_norm with edge_weight). Row t: its in-edges in input order, then its self loop; entries of value 0 dropped.
// With ew == nullptr and in-degree <= 7 these are build_ell's non-padding entries, bit for bit.
int build_csr(const int64_t* ei, const float* ew, int64_t E, int N, std::vector<int32_t>& rowptr,
              std::vector<int32_t>& cols, std::vector<float>& vals) {
  const int64_t* src = ei;
  const int64_t* dst = ei + E;
  for (int64_t e = 0; e < E; ++e) {
    if (src[e] < 0 || src[e] >= N || dst[e] < 0 || dst[e] >= N)
      return fail(SMAML_EINVAL, "edge " + std::to_string(e) + " (" + std::to_string(src[e]) + " -> " +
                                    std::to_string(dst[e]) + ") references a node outside [0, num_nodes)");
    if (ew && !(ew[e] >= 0.f && std::isfinite(ew[e])))
      return fail(SMAML_EINVAL, "edge " + std::to_string(e) + " (" + std::to_string(src[e]) + " -> " +
                                    std::to_string(dst[e]) + ") has a negative, NaN or infinite weight");
  }
  if (E + (int64_t)N > INT32_MAX) return fail(SMAML_EINVAL, "the graph has more than 2^31 - 1 entries");
  std::vector<float> loop(N, 1.f);  // add_remaining_self_loops: the last input loop's weight, else 1
  if (ew)
    for (int64_t e = 0; e < E; ++e)
      if (src[e] == dst[e]) loop[src[e]] = ew[e];
  std::vector<double> deg(N);
  for (int i = 0; i < N; ++i) deg[i] = loop[i];
  for (int64_t e = 0; e < E; ++e)
    if (src[e] != dst[e]) deg[dst[e]] += ew ? (double)ew[e] : 1.0;
  std::vector<float> dinv(N);
  for (int i = 0; i < N; ++i) {
    const float d = (float)deg[i];
    dinv[i] = d > 0.f ? 1.f / std::sqrt(d) : 0.f;
  }
  auto value = [&](int64_t s, float w, int64_t t) { return (dinv[s] * w) * dinv[t]; };
  rowptr.assign((size_t)N + 1, 0);
  for (int64_t e = 0; e < E; ++e)
    if (src[e] != dst[e] && value(src[e], ew ? ew[e] : 1.f, dst[e]) != 0.f) ++rowptr[dst[e] + 1];
  for (int i = 0; i < N; ++i) {
    if (value(i, loop[i], i) != 0.f) ++rowptr[i + 1];
    rowptr[i + 1] += rowptr[i];
  }
  cols.assign((size_t)rowptr[N], 0);
  vals.assign((size_t)rowptr[N], 0.f);
  std::vector<int32_t> pos(rowptr.begin(), rowptr.end() - 1);
  for (int64_t e = 0; e < E; ++e) {
    const int64_t s = src[e], t = dst[e];
    if (s == t) continue;
    const float v = value(s, ew ? ew[e] : 1.f, t);
    if (v == 0.f) continue;
    cols[pos[t]] = (int32_t)s;
    vals[pos[t]++] = v;
  }
  for (int i = 0; i < N; ++i) {
    const float v = value(i, loop[i], i);
    if (v == 0.f) continue;
    cols[pos[i]] = i;
    vals[pos[i]++] = v;
  }
  return SMAML_OK;
}

// The ELL's non-zero entries as CSR, in the ELL's order (what the transpose and the graph's counters walk).
void ell_to_csr(int N, const std::vector<int32_t>& ec, const std::vector<float>& ev, std::vector<int32_t>& rowptr,
                std::vector<int32_t>& cols, std::vector<float>& vals) {
  rowptr.assign((size_t)N + 1, 0);
  cols.clear();
  vals.clear();
  for (int t = 0; t < N; ++t) {
    for (int e = 0; e < ELLW; ++e)
      if (ev[(size_t)t * ELLW + e] != 0.f) {
        cols.push_back(ec[(size_t)t * ELLW + e]);
        vals.push_back(ev[(size_t)t * ELLW + e]);
      }
    rowptr[t + 1] = (int32_t)cols.size();
  }
}

// A_hat^T as CSR from A_hat's CSR: entry (t, e) (row t gathers column cols[e] with weight vals[e]) becomes an
// entry of row cols[e] of the transpose, in ascending t and, within t, in stored order (fixed order)
void csr_transpose(int N, const std::vector<int32_t>& rowptr, const std::vector<int32_t>& cols,
                   const std::vector<float>& vals, std::vector<int32_t>& tp, std::vector<int32_t>& tc,
                   std::vector<float>& tv) {
  tp.assign((size_t)N + 1, 0);
  for (int32_t j : cols) ++tp[j + 1];
  for (int i = 0; i < N; ++i) tp[i + 1] += tp[i];
  tc.resize(tp[N]);
  tv.resize(tp[N]);
  std::vector<int32_t> pos(tp.begin(), tp.end() - 1);
  for (int t = 0; t < N; ++t)
    for (int32_t e = rowptr[t]; e < rowptr[t + 1]; ++e) {
      const int j = cols[e];
      tc[pos[j]] = t;
      tv[pos[j]] = vals[e];
      ++pos[j];
    }
}

// one kernel per timing category (bench roofline = one kernel's launches)
// (the *_WALL categories: the wall time of a sweep whose diagonals ran as concurrent row chunks on side
// streams -- events on the caller's stream around the fork / join -- beside the per-chunk kernel times)
enum Cat { C_GCN = 0, C_FWD, C_FWD_DUAL, C_HEAD, C_HEAD_DH, C_BWD, C_BWD_DUAL, C_WGRAD, C_WGRAD_RED, C_MISC, C_XG, C_DGSUM,
           C_FWD_WALL, C_FWD_DUAL_WALL, C_BWD_WALL, C_BWD_DUAL_WALL, NCAT };

// Live per-category kernel timing with HIP events on the launch stream (bench roofline).
struct Timer {
  bool on = false;
  struct Rec {
    int cat;
    hipEvent_t a, b;
    double flops;
  };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  double ms[NCAT] = {};
  double flops[NCAT] = {};
  int64_t count[NCAT] = {};
  hipEvent_t get() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
};

// Pinned host staging ring for small host -> device uploads (window pointer tables, task ids):
// each upload takes the next slot, waits only for that slot's previous copy (event), then issues
// an async copy on the caller's stream -- no stream drain, the queue keeps running.
struct Staging {
  static constexpr int NSLOT = 4;
  char* host[NSLOT] = {};
  hipEvent_t evt[NSLOT] = {};
  int64_t cap = 0;  // bytes per slot
  int next = 0;
  int upload(hipStream_t s, void* dev, const void* src, int64_t bytes) {
    if (bytes > cap) {
      TRY(release());
      const int64_t c = std::max<int64_t>(bytes, 8192);
      for (int i = 0; i < NSLOT; ++i) {
        HIP_TRY(hipHostMalloc((void**)&host[i], c, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&evt[i], hipEventDisableTiming));
      }
      cap = c;
    }
    const int i = next;
    next = (next + 1) % NSLOT;
    HIP_TRY(hipEventSynchronize(evt[i]));  // this slot's previous copy has been consumed
    std::memcpy(host[i], src, bytes);
    HIP_TRY(hipMemcpyAsync(dev, host[i], bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(evt[i], s));
    return SMAML_OK;
  }
  int release() {
    for (int i = 0; i < NSLOT; ++i) {
      if (evt[i]) {
        HIP_TRY(hipEventSynchronize(evt[i]));
        HIP_TRY(hipEventDestroy(evt[i]));
      }
      if (host[i]) HIP_TRY(hipHostFree(host[i]));
      evt[i] = nullptr;
      host[i] = nullptr;
    }
    cap = 0;
    return SMAML_OK;
  }
};

}  // namespace

// The build-time defaults of the run-time knobs, by name (kernels.h Knobs; smaml_set_option changes them).
static Knobs default_knobs() {
  Knobs k;
  k.bwd_big_min = SMAML_BWD_BIG_MIN;
  k.bwdd_big_min = SMAML_BWDD_BIG_MIN;
  k.split_max = SMAML_SPLIT_MAX;
  k.wgrad_group_max_rows = SMAML_WGRAD_GROUP_ROWS;
  k.wgrad_group_wgs = SMAML_WGRAD_GROUP_WGS;
  k.gcn_fused = SMAML_GCN_FUSED;
  k.gate_img = SMAML_GATE_IMG;
  k.wgrad_wide = 1;
  k.wgrad_pair = SMAML_WGRAD_PAIR;
  k.bwdd_remap = SMAML_BWDD_REMAP_DEFAULT;
  k.small_kw = SMAML_SMALL_KW;
  k.gcn_dedup = 1;
  k.xg_dedup = SMAML_XG_DEDUP_DEFAULT;
  k.wgrad_dedup = SMAML_WGRAD_DEDUP_DEFAULT;
  k.bptt_streams = SMAML_BPTT_STREAMS_DEFAULT;
  k.fwd_streams = SMAML_FWD_STREAMS_DEFAULT;
  k.f_compact = SMAML_F_COMPACT_DEFAULT;
  return k;
}

// Host-timed phases of one smaml_adapt_steps call (smaml_adapt_phases): workspace reserve, feature-cache
// allocation, the batched cache fill, the step loop. The last two are enqueue times unless the option
// adapt_phase_sync is on (then each ends with a stream sync and includes the GPU time).
enum { AD_RESERVE = 0, AD_ALLOC, AD_FILL, AD_STEPS, AD_NPH };
struct AdPhases {
  double ms[AD_NPH] = {};
  int64_t filled = 0;  // windows computed by a per-step GCN pass (not the batched fill)
};

struct smaml_ctx {
  smaml_dims dims{};
  Dims d{};
  ParamOff po{};
  GcnOff go{};
  int device = 0;
  // Device memory the context owns is a HipBuf (devbuf.h); every other device pointer here aliases one.
  // The graph, all five set or none (smaml_set_graph): the normalised ELL (int32 columns, float values)
  // and A_hat^T as CSR (GCNConv backward's aggregation of the t = 0 rows)
  HipBuf ell_c, ell_v, tr_p, tr_c, tr_v;
  // The other form (smaml_set_graph_weighted): A_hat as CSR with its edge weights folded in, no degree limit.
  // graph_form says which of the two the entry points read (tr_* belongs to it); the other's buffers stay
  // allocated. graph_stats: smaml_graph_stats [1] .. [4].
  HipBuf csr_p, csr_c, csr_v;
  int graph_form = 0;  // 0 none, 1 ELL, 2 CSR
  int64_t graph_stats[5] = {};
  HipBuf bw_scratch;  // GCNConv backward: [rows][max(cin, cout)] x 2 floats
  // smaml_backward_base: conv1..conv3's recomputed activations [3][R][Hc], two gradient buffers
  // [2][R][max(Hc, Cin0)] and the samples' inputs in one piece [R][Cin0], R = nsamples*T*N (grows only)
  HipBuf bg_buf;
  int dx0_fused = 1;  // smaml_set_option("dx0_fused"): k_lstm_dx0 (1) or the GEMM + relu_mask + copies it replaces (0)
  // smaml_adapt_steps_full (grows only): conv1..conv3's kept outputs [3][R][Hc], two gradient buffers
  // [2][R][Hc], the t = 0 rows' raw products [B*N][Hc], the samples' inputs [R][Cin0] (B > 1) and the GCN
  // gradient [Pg], R = B*T*N
  HipBuf af_buf;
  int gcn_keep = 1;      // smaml_set_option("gcn_keep"): the forward keeps h1..h3 (1) or the backward recomputes them (0)
  // smaml_set_option("gcn_dz_fused"): k_gcn_dz (1) or GEMM + gather + mask per layer (0). Off by default: at
  // config-4 shapes the fused form measured 0.8 % SLOWER per step (1.307 against 1.297 ms, outside both spreads;
  // profiles/adapt_full_bench.log)
  int gcn_dz_fused = 0;
  int64_t af_stats[6] = {};  // smaml_adapt_full_stats: counters of the last smaml_adapt_steps_full call
  // smaml_meta_step_base's base stage (grows only): the stage's gradient rows [Z][R][Hc], one task's recomputed
  // conv1..conv3 outputs [3][R][Hc], a gradient buffer [R][Hc] and its windows side by side [R][Cin0] (R = B*T*N),
  // the row sums S and R S [2][Z][(2B + T - 2) N][4H], the stage's and the call's per-task gradients [2][Z][Pg]
  HipBuf mb_buf;
  // smaml_set_option("meta_base_dedup"): consecutive-window steps run the base stage over their distinct stream
  // rows (1) or over every sample row like the other steps (0). On by default: at config-2 shapes, 2 tasks, K = 5,
  // B = 32, order 2 the call measured 257.7 ms against 288.3 ms per-sample, outside both spreads (smaml_meta_step:
  // 217.3 ms; profiles/meta_base_bench.log)
  int meta_base_dedup = 1;
  int64_t mb_stats[6] = {};  // smaml_meta_base_stats: counters of the last smaml_meta_step_base call
  const float* gcn = nullptr;
  // Loss weights (smaml_set_loss_weights): lw_sets tables [Hf*N][C] in lw_buf; the set index of each region of
  // the running smaml_adapt_steps_multi call in lw_zset; node weights [N] of the forecast score sums in sw_buf
  // (smaml_set_score_weights). lw_count: smaml_loss_stats [2] .. [5]. None of these lives in the arena: they
  // survive smaml_reserve, smaml_set_tasks and the graph and parameter setters.
  HipBuf lw_buf, lw_zset, sw_buf;
  int lw_sets = 0;
  bool sw_set = false;
  int64_t lw_count[4] = {};
  // workspace
  HipBuf arena;
  int zb_cap = 0, z_cap = 0;
  Work w{};
  float* fast = nullptr;
  float* grad = nullptr;
  HipBuf scratch_loss;  // [(steps+1)*Z] floats, the fallback when the caller passes no buffer
  // device pointer table for sample windows (uploaded through the pinned staging ring)
  HipBuf xtab;  // never index directly: xtab_at (the table moves when it grows)
  int64_t xtab_n = 0;  // entries of the last upload_xtab
  Staging stage;
  // kernel-variant launch counters and run-time tile knobs (smaml_variant_counts / smaml_set_option)
  int64_t vcount[NVAR] = {};
  Knobs kn = default_knobs();
  int n_cu = 256;  // compute units of the device (smaml_create)
  int keep_max = -1;  // cap on kept second-order steps (-1: SMAML_KEEP env or all that fit)
  // tasks
  std::vector<const float*> feats;
  std::vector<int> t_total;
  Timer tm;
  // second-order state
  bool so_cap = false;
  float *so_u = nullptr, *so_hu = nullptr;
  HipBuf so_theta, so_grad, so_norm, so_coef;  // float; all four set or none (ensure_so_store)
  HipBuf so_F;  // float [K][Z][T][M][Hc] GCN features of every inner step (empty: recompute)
  int so_f_store = 1;  // smaml_set_option("so_f_store"): 0 = never keep them (the sweep asks run_gcn again)
  std::vector<int8_t> so_fc;  // per inner step: whether run_gcn wrote its so_F slot compact (Work::fcompact)
  float* F_main = nullptr;  // the workspace's own F buffer
  // batch-1 adaptation: GCN features per window of task 0 (the frozen GCN stack without dropout
  // is a pure function of the window, F2), filled on first use and reused by later epochs.
  // Invalidated by smaml_set_graph / _set_gcn_params / _set_tasks.
  HipBuf gcn_wimg;  // pre-split GCN weight images of the fused t >= 1 GCN (kernels_gcn.hip)
  HipBuf gimg_buf;  // pre-split gate-GEMM weight images (prep_gate_images)
  HipBuf bimg_buf;  // pre-split BPTT weight images (prep_bwd_images; small-grid BPTT)
  HipBuf xg_buf;    // small-grid forward: layer 0's hoisted input projection (run_lstm)
  HipBuf xgd_buf;   // big-tile forward: layer 0's projection per distinct stream row (xgd_scratch)
  // grid-barrier state of the bookkeeping kernels (kernels.h GridBar): device words [3], the pinned
  // device-mapped error flag a timed-out waiter sets, the wait bound and the launch form
  HipBuf bar;
  int* bar_err_host = nullptr;
  int* bar_err_dev = nullptr;
  int64_t bar_timeout_us = 4000000;  // smaml_set_option("barrier_timeout_us")
  int bar_fused = 1;                 // smaml_set_option("grid_barrier"): 0 = two launches per kernel
  int bar_oversize = 0;              // smaml_set_option("barrier_oversize"): debug, never co-resident
  uint64_t wall_khz = 0;             // wall_clock64 rate
  struct AdCache {
    HipBuf F;                    // float [valid.size()][T][N][Hc]
    std::vector<uint8_t> valid;  // per window start the cache has a slot for
  };
  std::vector<AdCache> ad;         // per task of smaml_set_tasks (smaml_adapt_steps uses task 0's)
  int ad_group = -1;               // smaml_set_option("adapt_group"): regions per lockstep launch set (0: all;
                                   // -1: the measured plan, ad_group_size)
  int ad_gcn_batch = 32;           // windows per GCN pass when filling the cache (<= 1: one per step)
  int ad_phase_sync = 0;           // smaml_set_option("adapt_phase_sync"): sync at the phase boundaries
  AdPhases ad_ph;                  // host-timed phases of the last smaml_adapt_steps (smaml_adapt_phases)
  // Per-stream GCN feature cache of the meta-step (smaml_set_option("gcn_stream_cache")): the frozen base without
  // GCN dropout gives stream row r of a task the same features in every window, inner step and meta-step (F2, F3),
  // so each row is computed once -- as a window's t = 0 row (graph gather, table t0) and as a t >= 1 row (no
  // neighbours, table t1) -- and consecutive-window steps gather their F from the tables (run_gcn_cached).
  // Keyed by stream pointer and length: entries survive smaml_set_tasks (task groups rotate every meta-step).
  struct GcEntry {
    const float* key = nullptr;
    int t_total = 0;
    HipBuf tab;                   // float [2][t_total][N][Hc]: t0, then t1
    std::vector<uint8_t> f0, f1;  // per stream row: filled (host; the fills are enqueued, gc_ev behind them)
    int64_t last_set = 0;         // gc_gen of the last meta-step that used the entry
  };
  std::vector<std::unique_ptr<GcEntry>> gc;
  int gc_on = 1;                // smaml_set_option("gcn_stream_cache")
  int64_t gc_budget_mb = -1;    // smaml_set_option("gcn_stream_cache_mb"): cap on the tables' bytes (-1: free HBM only)
  int64_t gc_gen = 0;           // meta-steps that asked for the cache
  hipStream_t gc_stream = nullptr;  // the stream the last fills were enqueued on (compared, never used)
  hipEvent_t gc_ev = nullptr;       // recorded behind them
  bool gc_ev_set = false;
  HipBuf gc_ptrs;               // device pointer table of a fill's t >= 1 runs
  // the running step's view of the cache (meta-step only; tab null: run_gcn computes the features itself)
  struct GcStep {
    const float* const* tab = nullptr;  // device [Z][2] (launch_gcn_cache_gather)
    GcEntry* const* ent = nullptr;      // host [Z]
    const int32_t* w0 = nullptr;        // host [Z]: each task's first window
    bool sweep = false;                 // the second-order sweep's visit of a step the inner loop ran
  } gc_cur;
  float *Hs_main = nullptr, *Cs_main = nullptr, *Gs_main = nullptr;  // the workspace's own activations
  // primal of the last inner steps kept for the second-order sweep (ensure_keep): slot 0 adds
  // dG + dh to the workspace's Hs/Cs/Gs, slot i >= 1 holds Hs/Cs/Gs/dG/dh of its own
  std::vector<HipBuf> keep_mem;
  int keep_n = 0;
  int64_t keep_rows = 0;  // rows * L the slots were sized for
  int keep_tried_K = -1;
  int keep_want = 0;  // slots the current second-order meta-step may use (<= keep_n)
  int keep_last = 0;  // slots the last second-order meta-step used
  // train-mode dropout (smaml_set_dropout / smaml_set_task_ids); p = 0: off
  float p_gcn = 0.f, p_lstm = 0.f;
  uint32_t drop_seed = 0;
  std::vector<int32_t> task_ids;  // global id of each task of smaml_set_tasks (default: its index)
  int* task_id_dev = nullptr;     // [z_cap] (arena)
  int64_t keep_tried_rows = -1;
  // activations of the last smaml_forward / smaml_lstm_forward (single task, act_B samples);
  // -1 once anything else has used the workspace (the backward consumes them: dG in place)
  int act_B = -1;
  // smaml_forecast's own buffers, sized from its pass size (grow only, never part of the arena, so a
  // forecast leaves the workspace and everything saved in it alone): the h / c rings of the inference
  // forward, the pass's GCN features and GCN ping-pong scratch, layer 0's projection per distinct stream
  // row, the pass's predictions when the caller wants only the sums, the skill partials and the scale
  HipBuf fc_ring;           // float [2][L][2][M][H]: the h ring, then the c ring
  HipBuf fc_F;              // [T][M][Hc], or the distinct rows only (consecutive passes)
  HipBuf fc_gcnA, fc_gcnB;  // all or none
  HipBuf fc_xg;             // [(2B + T - 2) N][4H]
  HipBuf fc_pred;           // [M][HfC]
  HipBuf fc_part;           // [skill_blocks][HfC][3]
  HipBuf fc_scale;          // [C]
  // smaml_forecast_ensemble shares the buffers above (fc_part holds 4 sums per entry there) and adds the
  // members' rings and the pass's member predictions
  HipBuf ens_ring;          // float [2][L][2][G][M][H], G = members per launch set
  HipBuf ens_pred;          // [E][M][HfC]
  bool ens_lds_set = false; // k_ens_stats's dynamic-LDS limit raised on this context's device (ens_stats_prepare)
  int ens_share = 1;        // smaml_set_option("ens_share"): layer 0 of the LSTM once for all members (p_gcn = 0)
  int ens_group = -1;       // smaml_set_option("ens_group"): members per launch set (0: all; -1: ens_group_size)
  // smaml_forecast_rollout shares fc_ring, fc_F (a run's features, time-major), fc_gcnA / B, fc_pred, fc_part
  // and fc_scale, and adds the origins' private sequences, layer 0's projection slot table with the t = 0
  // block behind it, the t = 0 rows' features and (no traj) one cycle's appended rows
  HipBuf ro_seq;            // [B][T + (R - 1) s][N][Cin]
  HipBuf ro_xg;             // [S + 1][M][4H]: slot rho % S of private row rho, then the t = 0 block
  HipBuf ro_F0;             // [M][Hc]
  HipBuf ro_blk;            // [B][s][N][C]
  int roll_reuse = 1;       // smaml_set_option("roll_reuse"): only the appended rows get features and projection
  int64_t ro_stats[5] = {}; // smaml_rollout_stats: counters of the last smaml_forecast_rollout call
  // smaml_forecast_rollout_ensemble shares fc_F, fc_gcnA / B, fc_part, fc_scale, ens_ring and ens_pred, and adds
  // the members' private sequences and slot tables, the observed rows' projection that all members read, the
  // t = 0 rows' features and (no member_traj) the pass's trajectories
  HipBuf re_seq;            // [G][B][T + (R - 1) s][N][Cin]
  HipBuf re_xg;             // [S][G][M][4H]: slot rho % S of appended row rho, per member; then [G][M][4H], t = 0
  HipBuf re_obs;            // [T][M][4H]: observed row rho (shared by the members); then [M][4H], cycle 0's t = 0
  HipBuf re_F0;             // [G][M][Hc]
  HipBuf re_traj;           // [E][B][R][s][N][C]
  bool rens_lds_set = false;      // k_rens_stats's dynamic-LDS limit raised (rens_stats_prepare)
  int64_t roll_ens_budget_mb = 32768; // smaml_set_option("roll_ens_budget_mb"): MiB a member group may take (measured:
                                      // 16 members at once 10 % faster than one at a time at config-2 shapes)
  int64_t re_stats[7] = {}; // smaml_rollout_ensemble_stats
  // side streams of the row-chunked BPTT (knob bptt_streams) and their fork / join events
  hipStream_t cs[4] = {};
  hipEvent_t fork_ev = nullptr, join_ev[4] = {};
  // RCCL communicator (smaml_comm_init), opaque; created non-blocking when the library allows it
  void* comm = nullptr;
  int comm_nb = 0;
  int64_t comm_timeout_ms = 120000;  // smaml_set_option("comm_timeout_ms")
};

namespace {

// The live graph as the launchers take it (kernels.h GraphView): the form and the tables of A_hat and A_hat^T.
GraphView graph_view(smaml_ctx* c) {
  GraphView g;
  g.form = c->graph_form;
  g.ell_c = c->ell_c.as<int32_t>();
  g.ell_v = c->ell_v.as<float>();
  g.csr_p = c->csr_p.as<int32_t>();
  g.csr_c = c->csr_c.as<int32_t>();
  g.csr_v = c->csr_v.as<float>();
  g.tr_p = c->tr_p.as<int32_t>();
  g.tr_c = c->tr_c.as<int32_t>();
  g.tr_v = c->tr_v.as<float>();
  g.csr_launches = &c->graph_stats[3];
  return g;
}

int ensure_device(smaml_ctx* c) {
  HIP_TRY(hipSetDevice(c->device));
  return SMAML_OK;
}

// Free HBM that a best-effort buffer must leave beyond its own size (HipBuf::grow_if_room).
constexpr int64_t SO_F_MARGIN = 4ll << 30, AD_F_MARGIN = 8ll << 30, KEEP_MARGIN = 8ll << 30;

void free_keep(smaml_ctx* c) {
  if (c->keep_mem.empty()) return;
  c->keep_mem.clear();
  c->keep_n = 0;
  c->keep_rows = 0;
  c->keep_tried_K = -1;
  c->keep_tried_rows = -1;
}

// Drops the adaptation feature cache.
void ad_cache_drop(smaml_ctx* c) {
  c->ad.clear();  // (each slot's buffer is released after a device sync, devbuf.h)
}

// Free HBM the per-stream GCN feature cache leaves (after the kept slots took theirs), and how many meta-steps
// an entry may go unused before a stream that finds no room may take its place.
constexpr int64_t GC_MARGIN = 2ll << 30, GC_STALE = 64;

// Drops the per-stream GCN feature cache, tables and all.
void gc_drop(smaml_ctx* c) {
  c->gc.clear();
  c->gc_cur = {};
}

// New graph / GCN parameters / a stream rewritten in place: every cached row is stale; the tables stay allocated.
void gc_invalidate(smaml_ctx* c) {
  for (auto& e : c->gc) {
    std::fill(e->f0.begin(), e->f0.end(), (uint8_t)0);
    std::fill(e->f1.begin(), e->f1.end(), (uint8_t)0);
  }
}

// The cache entries of the registered tasks, ent [Z] (null: that stream has none), allocating best effort the
// tables of streams seen for the first time. Whether every task has one.
bool gc_prepare(smaml_ctx* c, int Z, std::vector<smaml_ctx::GcEntry*>& ent) {
  const Dims& d = c->d;
  ++c->gc_gen;
  ent.assign((size_t)Z, nullptr);
  int64_t held = 0;
  for (auto& e : c->gc) held += e->tab.cap;
  bool all = true;
  for (int z = 0; z < Z; ++z) {
    smaml_ctx::GcEntry* hit = nullptr;
    for (auto& e : c->gc)
      if (e->key == c->feats[z] && e->t_total == c->t_total[z]) hit = e.get();
    if (!hit) {
      const int64_t bytes = 2ll * c->t_total[z] * d.N * d.Hc * 4;
      auto fits = [&]() { return c->gc_budget_mb < 0 || held + bytes <= (c->gc_budget_mb << 20); };
      auto e = std::make_unique<smaml_ctx::GcEntry>();
      bool ok = fits() && e->tab.grow_if_room(bytes, GC_MARGIN);
      while (!ok) {  // no room: the stream no meta-step has used for longest gives its tables up, if long enough
        size_t old = c->gc.size();
        for (size_t i = 0; i < c->gc.size(); ++i)
          if (c->gc[i]->last_set + GC_STALE < c->gc_gen && (old == c->gc.size() || c->gc[i]->last_set < c->gc[old]->last_set))
            old = i;
        if (old == c->gc.size()) break;
        held -= c->gc[old]->tab.cap;
        c->gc.erase(c->gc.begin() + (std::ptrdiff_t)old);
        ok = fits() && e->tab.grow_if_room(bytes, GC_MARGIN);
      }
      if (!ok) {
        all = false;
        continue;
      }
      e->key = c->feats[z];
      e->t_total = c->t_total[z];
      e->f0.assign((size_t)e->t_total, 0);
      e->f1.assign((size_t)e->t_total, 0);
      held += bytes;
      hit = e.get();
      c->gc.push_back(std::move(e));
    }
    hit->last_set = c->gc_gen;
    ent[z] = hit;
  }
  return all;
}

int reserve(smaml_ctx* c, int Z, int B, bool so = false) {
  const int zb = Z * B;
  // per-task activation slabs are addressed with 32-bit offsets inside the kernels
  if ((int64_t)c->d.T * B * c->d.N * 4 * c->d.H >= (1ll << 31))
    return fail(SMAML_EINVAL, "batch too large: T*B*N*4H must stay below 2^31 per task");
  so = so || c->so_cap;
  if (zb <= c->zb_cap && Z <= c->z_cap && so == c->so_cap) return SMAML_OK;
  ad_cache_drop(c);  // a growing workspace takes precedence over the adaptation feature cache
  gc_drop(c);        // ... and over the meta-step's per-stream one
  const int zbc = std::max(zb, c->zb_cap), zc = std::max(Z, c->z_cap);
  const Dims& d = c->d;
  const int64_t rows = (int64_t)zbc * d.T * d.N;
  const int64_t G = 4 * d.H;
  const int64_t seq = (int64_t)zbc * d.N;
  int max_cin = std::max(d.Hc, d.H);
  const int64_t wpart = std::max<int64_t>((int64_t)zc * G * (max_cin + d.H + 1) * SMAML_WGRAD_MAXSPLIT, 1 << 24);
  // loss partials per task: head_lblocks(M) for every per-task row count M <= seq
  const int64_t lblk =
      (int64_t)zc * (std::max<int64_t>(head_lblocks(d, (int)std::min<int64_t>(seq, SMAML_HEAD_SMALL_M)),
                                       (seq + 127) / 128) + 1);
  std::vector<std::pair<void**, int64_t>> parts;  // (dst, bytes)
  Work w{};
  parts.push_back({(void**)&w.F, rows * d.Hc * 4});
  parts.push_back({(void**)&w.Hs, rows * d.L * d.H * 4});
  parts.push_back({(void**)&w.Cs, rows * d.L * d.H * 4});
  parts.push_back({(void**)&w.Gs, rows * d.L * G * 4});  // gates, then dG in place (BPTT)
  parts.push_back({(void**)&w.dH, seq * d.H * 4});
  parts.push_back({(void**)&w.dc, seq * d.L * d.H * 4});
  parts.push_back({(void**)&w.gcnA, rows * d.Hc * 4});
  parts.push_back({(void**)&w.gcnB, rows * d.Hc * 4});
  parts.push_back({(void**)&w.pred, seq * d.HfC * 4});
  parts.push_back({(void**)&w.dpred, seq * d.HfC * 4});
  parts.push_back({(void**)&w.wpart, wpart * 4});
  parts.push_back({(void**)&w.lpart, lblk * 4});
  parts.push_back({(void**)&w.sqpart, (int64_t)(zc + 1) * SQB * 8});
  parts.push_back({(void**)&w.hTd, seq * d.H * 4});
  int* task_id_dev = nullptr;
  parts.push_back({(void**)&task_id_dev, (int64_t)zc * 4});
  float *fast = nullptr, *grad = nullptr;
  parts.push_back({(void**)&fast, (int64_t)zc * c->po.P * 4});
  parts.push_back({(void**)&grad, (int64_t)zc * c->po.P * 4});
  float *so_u = nullptr, *so_hu = nullptr;
  if (so) {
    parts.push_back({(void**)&w.RHs, rows * d.L * d.H * 4});
    parts.push_back({(void**)&w.RCs, rows * d.L * d.H * 4});
    parts.push_back({(void**)&w.RGs, rows * d.L * G * 4});
    parts.push_back({(void**)&w.RdH, seq * d.H * 4});
    parts.push_back({(void**)&w.Rdc, seq * d.L * d.H * 4});
    parts.push_back({(void**)&w.Rdpred, seq * d.HfC * 4});
    parts.push_back({(void**)&w.RhTd, seq * d.H * 4});
    parts.push_back({(void**)&so_u, (int64_t)zc * c->po.P * 4});
    parts.push_back({(void**)&so_hu, (int64_t)zc * c->po.P * 4});
  }
  int64_t total = 0;
  for (auto& p : parts) total += (p.second + 255) / 256 * 256;
  c->act_B = -1;
  free_keep(c);
  if (c->arena.grow(total) != hipSuccess) {
    c->zb_cap = c->z_cap = 0;  // no workspace: the next call sizes it afresh
    return fail(SMAML_ENOMEM, "hipMalloc of " + std::to_string(total) + " B workspace failed");
  }
  char* arena = c->arena.as<char>();
  int64_t off = 0;
  for (auto& p : parts) {
    *p.first = arena + off;
    off += (p.second + 255) / 256 * 256;
  }
  w.wpart_floats = wpart;
  c->w = w;
  c->task_id_dev = task_id_dev;
  c->fast = fast;
  c->grad = grad;
  c->zb_cap = zbc;
  c->z_cap = zc;
  c->so_cap = so;
  c->F_main = w.F;
  c->Hs_main = w.Hs;
  c->Cs_main = w.Cs;
  c->Gs_main = w.Gs;
  c->w.dG = w.Gs;
  c->so_u = so_u;
  c->so_hu = so_hu;
  HIP_TRY(hipMemset(grad, 0, (size_t)zc * c->po.P * 4));
  HIP_TRY(hipMemset(fast, 0, (size_t)zc * c->po.P * 4));
  if (so_hu) HIP_TRY(hipMemset(so_hu, 0, (size_t)zc * c->po.P * 4));
  return SMAML_OK;
}

// Per-step stores of the second-order sweep: theta_k and g_k [K][Z][P], |g_k| and the
// clip coefficient [K][Z].
int ensure_so_store(smaml_ctx* c, int K, int Z, int B, bool cached) {
  // GCN features of each inner step, kept for the second-order sweep (weight-independent, F2).
  // Best effort: without room the sweep recomputes them. cached: every inner step of this meta-step is served
  // from the per-stream GCN feature cache, which serves the sweep too -- no store is made for it (one that is
  // already there and large enough is used: it costs nothing more).
  const int64_t fbytes = (int64_t)K * Z * B * c->d.T * c->d.N * c->d.Hc * 4;
  if (c->so_f_store && (!cached || c->so_F.cap >= fbytes))
    (void)c->so_F.grow_if_room(fbytes, SO_F_MARGIN);
  else
    (void)c->so_F.release();
  const int64_t nc = (int64_t)K * Z * 4, need = nc * c->po.P;
  HIP_TRY(grow_all<HipAlloc>({{&c->so_theta, need}, {&c->so_grad, need}, {&c->so_norm, nc}, {&c->so_coef, nc}}));
  return SMAML_OK;
}

// Primal activations of the last inner steps, kept for the second-order sweep so that its
// dual kernels run tangent-only for those steps (no primal recompute of the forward or the
// BPTT GEMMs). Slot 0 (step K-1) keeps the workspace's own Hs/Cs/Gs -- the query then runs in
// the tangent buffers -- and adds dG + dh; slot i >= 1 (step K-1-i) holds its own
// Hs/Cs/Gs/dG/dh. Best effort: as many slots as fit in free HBM with a margin, capped by the
// SMAML_KEEP environment variable (0 disables). Needs the steps' GCN features at hand: the per-step store
// (so_F) or, `cached`, the per-stream GCN feature cache.
int ensure_keep(smaml_ctx* c, int K, int Z, int B, bool cached) {
  const Dims& d = c->d;
  int want = c->so_F.ptr || cached ? K : 0;
  if (c->keep_max >= 0)
    want = std::min(want, c->keep_max);
  else if (const char* e = std::getenv("SMAML_KEEP"))
    want = std::min(want, std::max(0, std::atoi(e)));
  const int64_t rowsL = (int64_t)Z * B * d.T * d.N * d.L;
  c->keep_want = want;
  if (want <= c->keep_n && rowsL <= c->keep_rows) return SMAML_OK;
  // already as many as fit for a group at least this large: keep those slots (unequal task groups, e.g.
  // 8 + 7, would otherwise free and re-allocate every slot at every group change, seconds per meta-step)
  if (rowsL <= c->keep_rows && want <= c->keep_tried_K && rowsL <= c->keep_tried_rows) return SMAML_OK;
  free_keep(c);
  c->keep_tried_K = want;
  c->keep_tried_rows = rowsL;
  for (int i = 0; i < want; ++i) {
    HipBuf slot;  // [dG | dh] or [Hs | Cs | Gs | dG | dh]
    if (!slot.grow_if_room(rowsL * (i == 0 ? 5 : 11) * d.H * 4, KEEP_MARGIN)) break;
    c->keep_mem.push_back(std::move(slot));
  }
  c->keep_n = (int)c->keep_mem.size();
  c->keep_rows = rowsL;
  return SMAML_OK;
}

// Points the workspace's primal activation buffers at the workspace's own (slot < 0), at a
// kept slot, or (query, when slot 0 holds the workspace's own) at the tangent buffers.
enum { SET_MAIN = -1, SET_QUERY = -2 };
void use_primal(smaml_ctx* c, int slot) {
  Work& w = c->w;
  const int64_t rowsL = (int64_t)w.Z * w.B * c->d.T * c->d.N * c->d.L;
  const int64_t H = c->d.H;
  w.dh = nullptr;
  if (slot == SET_QUERY) {
    w.Hs = w.RHs;
    w.Cs = w.RCs;
    w.Gs = w.dG = w.RGs;
  } else if (slot < 0) {
    w.Hs = c->Hs_main;
    w.Cs = c->Cs_main;
    w.Gs = w.dG = c->Gs_main;
  } else if (slot == 0) {
    w.Hs = c->Hs_main;
    w.Cs = c->Cs_main;
    w.Gs = c->Gs_main;
    w.dG = c->keep_mem[0].as<float>();
    w.dh = w.dG + rowsL * 4 * H;
  } else {
    float* p = c->keep_mem[slot].as<float>();
    w.Hs = p;
    w.Cs = p + rowsL * H;
    w.Gs = p + rowsL * 2 * H;
    w.dG = p + rowsL * 6 * H;
    w.dh = p + rowsL * 10 * H;
  }
}

// Dropout masks of one forward pass (inner step / query `step`) for the Z tasks of the workspace.
int upload_task_ids(smaml_ctx* c, hipStream_t s, int Z) {
  std::vector<int32_t> ids(Z);
  for (int z = 0; z < Z; ++z) ids[z] = z < (int)c->task_ids.size() ? c->task_ids[z] : z;
  return c->stage.upload(s, c->task_id_dev, ids.data(), (int64_t)Z * 4);  // pinned ring: no stream drain
}

void set_step_drop(smaml_ctx* c, int step) {
  Drop dr{};
  auto thr = [](float p) { return (uint32_t)std::min<double>(std::llround((double)p * 16777216.0), 16777216.0); };
  dr.seed = c->drop_seed;
  dr.step = step;
  dr.thr_gcn = thr(c->p_gcn);
  dr.thr_lstm = thr(c->p_lstm);
  dr.sc_gcn = 1.f / (1.f - c->p_gcn);
  dr.sc_lstm = 1.f / (1.f - c->p_lstm);
  dr.task_id = c->task_id_dev;
  c->w.drop = dr;
}

int upload_xtab(smaml_ctx* c, hipStream_t s, const float* const* ptrs, int64_t n) {
  c->xtab_n = 0;
  HIP_TRY(c->xtab.grow(std::max<int64_t>(n, 1024) * (int64_t)sizeof(float*)));
  TRY(c->stage.upload(s, c->xtab.ptr, ptrs, n * (int64_t)sizeof(float*)));
  c->xtab_n = n;
  return SMAML_OK;
}

// Device address of entry i of the window table. The only way table pointers are formed: after the
// upload_xtab that wrote entry i (an upload may move the table, so a pointer taken before it could
// dangle -- the fault class of round 4's first gcn_dedup run).
int xtab_at(const smaml_ctx* c, int64_t i, const float* const** out) {
  if (i < 0 || i >= c->xtab_n)
    return fail(SMAML_EINVAL, "internal: window-table entry " + std::to_string(i) + " read before its upload (" +
                                  std::to_string(c->xtab_n) + " uploaded)");
  *out = c->xtab.as<const float*>() + i;
  return SMAML_OK;
}

void set_work(smaml_ctx* c, int Z, int B) {
  c->act_B = -1;  // any new use of the workspace ends the validity of saved activations
  c->w.Z = Z;
  c->w.B = B;
  c->w.M = B * c->d.N;
  c->w.lblocks = head_lblocks(c->d, c->w.M);
  c->w.F = c->F_main;
  c->w.primal_kept = 0;
  c->w.consec = 0;
  c->w.fcompact = 0;
  c->w.drop = Drop{};  // dropout only inside smaml_meta_step / smaml_adapt_steps (set_step_drop)
  c->w.lw = LossW{};   // loss weights only where an entry point asks for them (use_loss_weights)
  c->w.vcount = c->vcount;
  c->w.kn = c->kn;
  if (c->Hs_main) use_primal(c, SET_MAIN);
}

// The loss weights of a compute call that reads the registered tasks: more than one set must be one per task.
int check_loss_weights(const smaml_ctx* c, const char* who) {
  if (c->lw_sets > 1 && c->lw_sets != (int)c->feats.size())
    return fail(SMAML_ESTATE, std::string(who) + ": " + std::to_string(c->lw_sets) + " loss weight sets held but " +
                                  std::to_string(c->feats.size()) + " tasks registered (one set, or one per task)");
  return SMAML_OK;
}

// Points the workspace's head launches at the live table (after set_work, which clears it): task z of the launch
// reads set zset[z] (a device table), or set z without one; a single set is shared by every task.
void use_loss_weights(smaml_ctx* c, const int32_t* zset) {
  if (c->lw_sets <= 0) return;
  LossW& lw = c->w.lw;
  lw.w = c->lw_buf.as<float>();
  lw.zstride = c->lw_sets > 1 ? (int64_t)c->d.Hf * c->d.N * c->d.C : 0;
  lw.zset = c->lw_sets > 1 ? zset : nullptr;
  lw.count = c->lw_count;
}

// The node weights of the forecast score sums, or null; counts the launch that reads them.
const float* score_weights(smaml_ctx* c) {
  if (!c->sw_set) return nullptr;
  ++c->lw_count[3];
  return c->sw_buf.as<float>();
}

#define TIMED(c, s, cat, fl, stmt)                              \
  do {                                                           \
    if ((c)->tm.on) {                                            \
      hipEvent_t a_ = (c)->tm.get(), b_ = (c)->tm.get();         \
      (void)hipEventRecord(a_, s);                               \
      stmt;                                                      \
      (void)hipEventRecord(b_, s);                               \
      (c)->tm.recs.push_back({cat, a_, b_, (double)(fl)});       \
    } else {                                                     \
      stmt;                                                      \
    }                                                            \
  } while (0)

// Weight gradient = split-K GEMM (C_WGRAD) + fixed-order reduce (C_WGRAD_RED).
int fork_streams(smaml_ctx* c, hipStream_t s, int n);

// One weight gradient's split-K GEMM + reduce, in order on s.
void wgrad_run(smaml_ctx* c, hipStream_t s, double fl, WgradPlan& p) {
  TIMED(c, s, C_WGRAD, fl, launch_wgrad_gemm(s, p));
  TIMED(c, s, C_WGRAD_RED, 0, launch_wgrad_reduce(s, p));
}

void timed_wgrad(smaml_ctx* c, hipStream_t s, double fl, const float* A, int64_t a_zstride, int Mrows,
                 const float* B1, int64_t b1_zstride, int c1, const float* B2, int64_t b2_zstride, int c2, int64_t K,
                 int Mshift, float* grad, int64_t P, int64_t off_w1, int64_t off_w2, int64_t off_b1, int64_t off_b2,
                 bool with_bias = true, bool accumulate = false, int drop_layer = -1) {
  WgradPlan p;
  plan_wgrad(c->w, A, a_zstride, Mrows, B1, b1_zstride, c1, B2, b2_zstride, c2, K, Mshift, grad, P, off_w1, off_w2,
             off_b1, off_b2, with_bias, accumulate, p);
  p.drop = c->w.drop;  // B1 = drop(h_{drop_layer}) under LSTM dropout (input weights of layer >= 1)
  p.drop_layer = drop_layer;
  count_variant(c->w, V_WGRAD);
  if (p.wide) count_variant(c->w, V_WGRAD_WIDE);
  wgrad_run(c, s, fl, p);
}

// Tangent weight gradient of one LSTM layer as ONE split-K launch + ONE reduce:
//   R(dW) = R(dG)^T [x | h_{t-1}] + dG^T [Rx | Rh_{t-1}]   (both problems 4H x (cin + H)).
bool timed_wgrad_pair(smaml_ctx* c, hipStream_t s, double fl, const float* RdG, const float* dG, int64_t a_zstride,
                      int Mrows, const float* X, const float* RX, int64_t b1_zstride, int c1, const float* Hh,
                      const float* RHh, int64_t b2_zstride, int c2, int64_t K, int Mshift, float* grad, int64_t P,
                      int64_t off_w1, int64_t off_w2, int64_t off_b1, int64_t off_b2, int drop_layer) {
  WgradPlan p;
  plan_wgrad(c->w, RdG, a_zstride, Mrows, X, b1_zstride, c1, Hh, b2_zstride, c2, K, Mshift, grad, P, off_w1, off_w2,
             off_b1, off_b2, true, false, p);
  if (!pair_wgrad(p, c->w, dG, RX, RHh)) return false;  // the caller runs the two accumulating passes
  p.drop = c->w.drop;
  p.drop_layer = drop_layer;
  count_variant(c->w, V_WGRAD);
  if (p.wide) count_variant(c->w, V_WGRAD_WIDE);
  count_variant(c->w, V_WGRAD_PAIR);
  wgrad_run(c, s, fl, p);
  return true;
}

// Row chunks of a forward sweep (knob fwd_streams; 0 = auto: two when one problem's big-tile gate launch
// fills at most one round of the device's workgroup slots, e.g. config 5's one-task groups, where the
// chunks fill each other's tails; at config 2 a diagonal is ~9 rounds and chunking measured slower).
int fwd_chunks(const smaml_ctx* c) {
  const Work& w = c->w;
  // (only where the full diagonal runs the big tiles anyway; every chunked diagonal does)
  if ((int64_t)w.Z * w.M <= c->kn.wgrad_group_max_rows || !fwd_wave_big(c->d, w, c->po, std::min(c->d.L, c->d.T) - 1))
    return 1;
  if (c->kn.fwd_streams > 0) return c->kn.fwd_streams;
  const int64_t wgs = (int64_t)(w.M + 255) / 256 * ((c->d.H + 31) / 32) * w.Z;  // 256-row x 32-unit gate tiles
  return wgs <= 2LL * c->n_cu ? 2 : 1;
}

// Side streams for row chunks of the BPTT (knob bptt_streams): each waits for the work already on s.
int fork_streams(smaml_ctx* c, hipStream_t s, int n) {
  if (!c->fork_ev) HIP_TRY(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c->fork_ev, s));
  for (int i = 0; i < n; ++i) {
    if (!c->cs[i]) HIP_TRY(hipStreamCreateWithFlags(&c->cs[i], hipStreamNonBlocking));
    if (!c->join_ev[i]) HIP_TRY(hipEventCreateWithFlags(&c->join_ev[i], hipEventDisableTiming));
    HIP_TRY(hipStreamWaitEvent(c->cs[i], c->fork_ev, 0));
  }
  return SMAML_OK;
}
// the workspace as chunk ci's launches see it: launch counters once per diagonal (chunk 0's)
Work chunk_work(const Work& w, int ci) {
  Work q = w;
  if (ci > 0) q.vcount = nullptr;
  return q;
}

// a timing record of category cat from event a (recorded on s before a fork) to now on s (after the join)
void time_wall(smaml_ctx* c, hipStream_t s, hipEvent_t a, int cat, double fl) {
  if (!a) return;
  hipEvent_t b = c->tm.get();
  (void)hipEventRecord(b, s);
  c->tm.recs.push_back({cat, a, b, fl});
}

// s waits for everything issued on the side streams
int join_streams(smaml_ctx* c, hipStream_t s, int n) {
  for (int i = 0; i < n; ++i) {
    HIP_TRY(hipEventRecord(c->join_ev[i], c->cs[i]));
    HIP_TRY(hipStreamWaitEvent(s, c->join_ev[i], 0));
  }
  return SMAML_OK;
}

// The XgDedup-row-order scratch (k_xg_dedup tables / k_dg_rowsum sums) with room for `floats`, or null.
float* xgd_scratch(smaml_ctx* c, int64_t floats) {
  return c->xgd_buf.grow(floats * 4) == hipSuccess ? c->xgd_buf.as<float>() : nullptr;
}

// Whether this step's layer-0 input-weight gradient runs over distinct stream rows (wgrad_dedup).
bool wgrad_dedup_ok(const smaml_ctx* c) {
  const Work& w = c->w;
  return w.consec && c->kn.wgrad_dedup && w.B > 1 && !w.drop.gcn() && !w.drop.lstm();
}

// dW_ih0 (or its tangent) = S^T F_rows over the distinct stream rows of the step's consecutive windows:
// S = row sums of dGl (layer 0's dG or R(dG), k_dg_rowsum, in the scratch), then ONE gathered split-K
// GEMM into grad's W_ih0 block (no bias; written, not accumulated). False: no scratch (the caller runs
// the full-row form).
bool timed_wgrad_ih0_dedup(smaml_ctx* c, hipStream_t s, const float* dGl, float* grad) {
  const Dims& d = c->d;
  Work& w = c->w;
  const int64_t rows = xg_dedup_rows(w.B, d.T, d.N), TM = (int64_t)d.T * w.M;
  float* S = xgd_scratch(c, rows * 4 * d.H * w.Z);
  if (!S) return false;
  const LayerOff& lo = c->po.lay[0];
  TIMED(c, s, C_DGSUM, 0, launch_dg_rowsum(s, d, w, dGl, TM * 4 * d.H, S));
  WgradPlan p;
  plan_wgrad(w, S, rows * 4 * d.H, 4 * d.H, w.F, TM * lo.cin, lo.cin, nullptr, 0, 0, rows, 0, grad, c->po.P, lo.wih, -1,
             -1, -1, false, false, p);
  p.gather = WgGather{w.M, d.N, d.T, FastDiv((uint32_t)d.N), w.fcompact};
  count_variant(w, V_WGRAD);
  count_variant(w, V_WGRAD_DEDUP);
  if (p.wide) count_variant(w, V_WGRAD_WIDE);
  wgrad_run(c, s, 2.0 * w.Z * rows * 4 * d.H * lo.cin, p);
  return true;
}

// Whether a consecutive-window step's features may be stored compact (Work::fcompact, the distinct rows
// only, XgDedup order): every reader of F must then take those rows -- the forwards' layer-0 gates through
// the k_xg_dedup tables (every layer-0 diagonal on the big tiles; the tangent forward always reads them),
// the backwards' dW_ih0 through the gathered form (not the grouped small-grid launch) -- with the
// scratch for both tables reserved here, so neither reader can miss it later. Deterministic in the
// step's state; the tangent sweep reuses the flag recorded when a step's so_F slot was written (so_fc).
bool f_compact_ok(smaml_ctx* c, bool consec) {
  const Dims& d = c->d;
  const Work& w = c->w;
  const Knobs& kn = c->kn;
  // The compact rows of a task, (2B + T - 2) N, live in its [T][B N] slab of F (and of a kept so_F slot):
  // they fit iff (T - 2)(B - 1) >= 0. A window of ONE step shares no stream row with its neighbours, its
  // (2B - 1) N compact rows would run (B - 1) N rows past the slab -- into the next task's rows and, for the
  // last task, past the buffer.
  if (d.T < 2) return false;
  if (!consec || !kn.f_compact || !kn.gcn_dedup || !kn.xg_dedup || !kn.wgrad_dedup || w.B <= 1 || w.drop.gcn() ||
      w.drop.lstm() || (int64_t)w.Z * w.M <= kn.wgrad_group_max_rows)
    return false;
  for (int diag = 0; diag < d.T; ++diag)
    if (!fwd_wave_big(d, w, c->po, diag)) return false;
  return xgd_scratch(c, 2 * xg_dedup_rows(w.B, d.T, d.N) * 4 * d.H * w.Z) != nullptr;
}

// A consecutive-window step served from the per-stream GCN feature cache (c->gc_cur): the rows the step reads
// that the tables do not hold yet -- w0 .. w0 + B - 1 of t0, w0 + 1 .. w0 + B + T - 2 of t1 -- are computed in
// runs of consecutive stream rows by run_gcn's own kernels (a row's arithmetic does not depend on which rows share
// its launch: the t = 0 rows as N-row samples with the graph gather, layer by layer; the others by k_gcn_mlp's row-
// run form, or on the per-layer path as one pseudo-sample without neighbours), then one copy kernel lays F out
// as run_gcn would have (w.fcompact decided by the caller). Once a stream's rows are filled no GCN kernel runs.
int run_gcn_cached(smaml_ctx* c, hipStream_t s) {
  const Dims& d = c->d;
  Work& w = c->w;
  const smaml_ctx::GcStep& g = c->gc_cur;
  // the filled flags speak of work enqueued on the last fill's stream: another stream waits for it
  if (c->gc_ev_set && c->gc_stream != s) HIP_TRY(hipStreamWaitEvent(s, c->gc_ev, 0));
  struct Run {
    smaml_ctx::GcEntry* e;
    int a, n;  // stream rows a .. a + n - 1
  };
  std::vector<Run> r0, r1;
  auto missing = [](smaml_ctx::GcEntry* e, std::vector<uint8_t>& f, int lo, int hi, std::vector<Run>& out) {
    for (int r = lo; r < hi; ++r) {
      if (f[(size_t)r]) continue;
      f[(size_t)r] = 1;
      if (!out.empty() && out.back().e == e && out.back().a + out.back().n == r)
        ++out.back().n;
      else
        out.push_back({e, r, 1});
    }
  };
  struct Guard {  // an error below leaves rows marked that were never enqueued: forget them all
    smaml_ctx* c;
    bool done = false;
    ~Guard() {
      if (!done) gc_invalidate(c);
    }
  } guard{c};
  for (int z = 0; z < w.Z; ++z) {
    missing(g.ent[z], g.ent[z]->f0, g.w0[z], g.w0[z] + w.B, r0);
    if (d.T > 1) missing(g.ent[z], g.ent[z]->f1, g.w0[z] + 1, g.w0[z] + w.B + d.T - 1, r1);
  }
  const int64_t blk = (int64_t)d.N * d.Hc, xblk = (int64_t)d.N * d.Cin0;
  float* bufs[2] = {w.gcnA, w.gcnB};  // a run is at most B + T - 2 rows: within the step's own [Z B T N][Hc]
  const GraphView gv = graph_view(c);
  const bool fused = gcn_mlp_supported(d) && c->kn.gcn_fused;
  if (!r1.empty()) {
    std::vector<const float*> ptrs;
    for (const Run& r : r1) ptrs.push_back(r.e->key + (int64_t)r.a * xblk);
    HIP_TRY(c->gc_ptrs.grow(std::max<int64_t>((int64_t)ptrs.size(), 256) * (int64_t)sizeof(float*)));
    TRY(c->stage.upload(s, c->gc_ptrs.ptr, ptrs.data(), (int64_t)ptrs.size() * (int64_t)sizeof(float*)));
    const float* const* tab = c->gc_ptrs.as<const float*>();
    GcnWOff wo;
    for (int k = 0; k < 4; ++k) {
      wo.w[k] = c->go.w[k];
      wo.b[k] = c->go.b[k];
    }
    char* wimg = nullptr;
    if (fused) {
      HIP_TRY(c->gcn_wimg.grow(gcn_wimg_bytes(d)));
      wimg = c->gcn_wimg.as<char>();
      TIMED(c, s, C_MISC, 0, launch_gcn_wsplit(s, d, c->gcn, wo, wimg));
    }
    for (size_t i = 0; i < r1.size(); ++i) {
      const Run& r = r1[i];
      float* out = r.e->tab.as<float>() + ((int64_t)r.e->t_total + r.a) * blk;
      if (fused) {
        TIMED(c, s, C_GCN, 2.0 * r.n * d.N * d.Hc * (d.Cin0 + 3.0 * d.Hc),
              launch_gcn_mlp_run(s, d, 1, r.n, tab + i, c->gcn, wo, wimg, out));
        continue;
      }
      const float* src = nullptr;
      for (int k = 0; k < 4; ++k) {
        float* dst = k == 3 ? out : bufs[k & 1];
        TIMED(c, s, C_GCN, 2.0 * r.n * d.N * c->go.cin[k] * d.Hc,
              launch_gcn_layer(s, d, k, 1, 1, k == 0 ? tab + i : nullptr, src, dst, false, true, c->gcn + c->go.w[k],
                               c->gcn + c->go.b[k], c->go.cin[k], d.Hc, gv, r.n * d.N, 0, nullptr));
        src = dst;
      }
    }
  }
  for (const Run& r : r0) {  // t = 0 rows: r.n samples of N rows, one after another in the stream and in t0
    const float* src = r.e->key + (int64_t)r.a * xblk;
    for (int k = 0; k < 4; ++k) {
      float* dst = k == 3 ? r.e->tab.as<float>() + (int64_t)r.a * blk : bufs[k & 1];
      TIMED(c, s, C_GCN, 2.0 * r.n * d.N * c->go.cin[k] * d.Hc,
            launch_gcn_layer(s, d, k, r.n, 1, nullptr, src, dst, false, true, c->gcn + c->go.w[k], c->gcn + c->go.b[k],
                             c->go.cin[k], d.Hc, gv, d.N, d.N, nullptr));
      src = dst;
    }
  }
  int64_t rows = 0;
  for (const Run& r : r0) rows += r.n;
  for (const Run& r : r1) rows += r.n;
  if (w.vcount) w.vcount[V_GCN_CACHE_ROWS] += rows;
  if (rows > 0 || c->gc_stream != s) {
    if (!c->gc_ev) HIP_TRY(hipEventCreateWithFlags(&c->gc_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->gc_ev, s));
    c->gc_ev_set = true;
    c->gc_stream = s;
  }
  count_variant(w, V_GCN_CACHE);
  TIMED(c, s, C_MISC, 0, launch_gcn_cache_gather(s, d, w.Z, w.B, g.tab, w.F, w.fcompact != 0));
  HIP_TRY(hipGetLastError());
  guard.done = true;
  return SMAML_OK;
}

// GCN x4 (no_grad, F2): sample windows -> w.F [Z][T][M][Hc]. With the fused kernel (Hc = 256): the
// rows t >= 1 (no neighbours, F3) run all four convs in one launch (k_gcn_mlp, activations kept in
// registers), the t = 0 rows (ELL gather) four per-layer launches over N-row blocks.
// first_tab (device, [Z]: each task's first window pointer), given when every task's B windows start at
// consecutive stream rows (the caller checked the window table): the rows t >= 1 are then computed
// once per distinct stream row -- by the fused kernel (k_gcn_mlp dedup), or, on the per-layer path,
// as one (B + T - 1) N-row pseudo-sample per task without neighbours, expanded into F afterwards.
// fcompact >= 0: the caller decided the layout of F itself (smaml_forecast, whose readers are not the
// training step's: forecast_compact_ok).
int run_gcn(smaml_ctx* c, hipStream_t s, const float* const* xtab_dev, const float* const* first_tab = nullptr,
            int fcompact = -1) {
  const bool consec = first_tab != nullptr;
  const Dims& d = c->d;
  Work& w = c->w;
  w.fcompact = fcompact >= 0 ? fcompact : f_compact_ok(c, consec) ? 1 : 0;
  const bool served = consec && c->gc_cur.tab && fcompact < 0 && c->kn.gcn_dedup && w.B > 1 && !w.drop.gcn();
  // (a sweep step served from the cache lays the same step's features out again: counted once per step, as when
  // the sweep read them from the per-step store)
  const bool revisit = served && c->gc_cur.sweep;
  if (w.fcompact && !revisit) count_variant(w, V_F_COMPACT);
  if (served) {
    if (!revisit) count_variant(w, V_GCN_DEDUP);  // (each distinct stream row at most once, here once per stream)
    return run_gcn_cached(c, s);
  }
  const int rps = d.T * d.N;
  const int zb = w.Z * w.B;
  const float* src = nullptr;
  float* bufs[2] = {w.gcnA, w.gcnB};
  const GraphView gv = graph_view(c);
  if (gcn_mlp_supported(d) && c->kn.gcn_fused) {
    HIP_TRY(c->gcn_wimg.grow(gcn_wimg_bytes(d)));
    char* wimg = c->gcn_wimg.as<char>();
    GcnWOff wo;
    for (int k = 0; k < 4; ++k) {
      wo.w[k] = c->go.w[k];
      wo.b[k] = c->go.b[k];
    }
    // the GCN parameters may change between calls (smaml_set_gcn_params keeps the pointer): re-split
    TIMED(c, s, C_MISC, 0, launch_gcn_wsplit(s, d, c->gcn, wo, wimg));
    const bool dedup = consec && c->kn.gcn_dedup && w.B > 1 && !w.drop.gcn();
    if (dedup) count_variant(w, V_GCN_DEDUP);
    const double rows1 = dedup ? (double)w.Z * (w.B + d.T - 2) * d.N : (double)zb * (d.T - 1) * d.N;
    TIMED(c, s, C_GCN, 2.0 * rows1 * d.Hc * (d.Cin0 + 3.0 * d.Hc),
          launch_gcn_mlp(s, d, zb, w.B, xtab_dev, c->gcn, wo, wimg, w.F, &w.drop, dedup, w.fcompact));
    for (int k = 0; k < 4; ++k) {  // t = 0 rows: N-row blocks, masks indexed as rows of T*N-row samples
      const bool last = k == 3;
      float* dst = last ? w.F : bufs[k & 1];
      TIMED(c, s, C_GCN, 2.0 * zb * d.N * c->go.cin[k] * d.Hc,
            launch_gcn_layer(s, d, k, zb, w.B, k == 0 ? xtab_dev : nullptr, src, dst, last, true,
                             c->gcn + c->go.w[k], c->gcn + c->go.b[k], c->go.cin[k], d.Hc, gv,
                             d.N, d.N, &w.drop, rps));
      src = dst;
    }
    HIP_TRY(hipGetLastError());
    return SMAML_OK;
  }
  if (consec && c->kn.gcn_dedup && w.B > 1 && !w.drop.gcn()) {
    count_variant(w, V_GCN_DEDUP);
    const int rpsC = (w.B + d.T - 1) * d.N;  // stream rows w0 .. w0 + B + T - 2 of each task
    for (int k = 0; k < 4; ++k) {
      float* dst = bufs[k & 1];
      TIMED(c, s, C_GCN, 2.0 * w.Z * rpsC * c->go.cin[k] * d.Hc,
            launch_gcn_layer(s, d, k, w.Z, 1, k == 0 ? first_tab : nullptr, src, dst, false, true,
                             c->gcn + c->go.w[k], c->gcn + c->go.b[k], c->go.cin[k], d.Hc, gv,
                             rpsC, 0, nullptr));
      src = dst;
    }
    TIMED(c, s, C_GCN, 0, launch_gcn_expand(s, d, w.Z, w.B, src, w.F, w.fcompact));
    src = nullptr;
    for (int k = 0; k < 4; ++k) {  // t = 0 rows: N-row blocks with the ELL gather, as on the fused path
      const bool last = k == 3;
      float* dst = last ? w.F : bufs[k & 1];
      TIMED(c, s, C_GCN, 2.0 * zb * d.N * c->go.cin[k] * d.Hc,
            launch_gcn_layer(s, d, k, zb, w.B, k == 0 ? xtab_dev : nullptr, src, dst, last, true,
                             c->gcn + c->go.w[k], c->gcn + c->go.b[k], c->go.cin[k], d.Hc, gv,
                             d.N, d.N, &w.drop, rps));
      src = dst;
    }
    HIP_TRY(hipGetLastError());
    return SMAML_OK;
  }
  for (int k = 0; k < 4; ++k) {
    const bool last = k == 3;
    float* dst = last ? w.F : bufs[k & 1];
    TIMED(c, s, C_GCN, 2.0 * zb * rps * c->go.cin[k] * d.Hc,
          launch_gcn_layer(s, d, k, zb, w.B, k == 0 ? xtab_dev : nullptr, src, dst, last, true,
                           c->gcn + c->go.w[k], c->gcn + c->go.b[k], c->go.cin[k], d.Hc, gv,
                           rps, d.N, &w.drop));
    src = dst;
  }
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

// run_gcn for a step whose backward runs through the base (smaml_adapt_steps_full; one task, any B): w.F as
// run_gcn writes it, and conv1..conv3's outputs (post-ReLU, post-dropout) kept in h[k], per sample
// [s][T*N][Hc] -- what the GCN backward reads. Fused path: the keep variant of k_gcn_mlp stores the rows
// t >= 1 from its epilogues, and the t = 0 rows' per-layer launches read and write rows 0 .. N-1 of each
// sample in h[k] (sample stride T*N rows) instead of ping-ponging through N-row blocks. Per-layer path: layer
// k writes h[k] directly. Never dedup or compact: every sample keeps its own rows. Same per-row arithmetic as
// run_gcn. stats: [1] += fused keeping launches, [2] += per-layer keeping launches over all rows.
int run_gcn_keep(smaml_ctx* c, hipStream_t s, const float* const* xtab_dev, float* const h[3], int64_t* stats) {
  const Dims& d = c->d;
  Work& w = c->w;
  w.fcompact = 0;
  const int rps = d.T * d.N;
  const int zb = w.Z * w.B;
  const GraphView gv = graph_view(c);
  if (gcn_mlp_supported(d) && c->kn.gcn_fused) {
    char* wimg = c->gcn_wimg.as<char>();  // (grown by the caller before its first launch)
    GcnWOff wo;
    for (int k = 0; k < 4; ++k) {
      wo.w[k] = c->go.w[k];
      wo.b[k] = c->go.b[k];
    }
    TIMED(c, s, C_MISC, 0, launch_gcn_wsplit(s, d, c->gcn, wo, wimg));  // the base moved in the last step: re-split
    TIMED(c, s, C_GCN, 2.0 * zb * (d.T - 1) * d.N * d.Hc * (d.Cin0 + 3.0 * d.Hc),
          launch_gcn_mlp(s, d, zb, w.B, xtab_dev, c->gcn, wo, wimg, w.F, &w.drop, false, false, h[0]));
    stats[1] += 1;
    for (int k = 0; k < 4; ++k) {  // t = 0 rows: rows 0 .. N-1 of every sample
      const bool last = k == 3;
      TIMED(c, s, C_GCN, 2.0 * zb * d.N * c->go.cin[k] * d.Hc,
            launch_gcn_layer(s, d, k, zb, w.B, k == 0 ? xtab_dev : nullptr, k == 0 ? nullptr : h[k - 1],
                             last ? w.F : h[k], last, true, c->gcn + c->go.w[k], c->gcn + c->go.b[k], c->go.cin[k],
                             d.Hc, gv, d.N, d.N, &w.drop, rps, rps, rps));
    }
    HIP_TRY(hipGetLastError());
    return SMAML_OK;
  }
  for (int k = 0; k < 4; ++k) {
    const bool last = k == 3;
    TIMED(c, s, C_GCN, 2.0 * zb * rps * c->go.cin[k] * d.Hc,
          launch_gcn_layer(s, d, k, zb, w.B, k == 0 ? xtab_dev : nullptr, k == 0 ? nullptr : h[k - 1],
                           last ? w.F : h[k], last, true, c->gcn + c->go.w[k], c->gcn + c->go.b[k], c->go.cin[k],
                           d.Hc, gv, rps, d.N, &w.drop));
    stats[2] += 1;
  }
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

// Pre-split images of theta's gate-GEMM weights for this forward (launch_split_gate; the fast
// weights change every inner step, so every forward re-splits them: a few microseconds).
int prep_gate_images(smaml_ctx* c, hipStream_t s, const float* theta, int64_t tstride, const float* U = nullptr) {
  const Dims& d = c->d;
  Work& w = c->w;
  w.gimg = GateImgs{};
  w.gimg_src = nullptr;
  w.gimg_u_src = nullptr;
  if (!c->kn.gate_img || w.drop.lstm()) return SMAML_OK;  // (the dropout kernels load f32 weights)
  GateImgs gi{};
  const int64_t per = gate_img_bytes(d, &gi) * w.Z;
  // no room: the kernels load and split the f32 weights themselves
  if (c->gimg_buf.grow(per * (U ? 2 : 1)) != hipSuccess) return SMAML_OK;
  gi.th = c->gimg_buf.as<char>();
  TIMED(c, s, C_MISC, 0, launch_split_gate(s, d, c->po, theta, tstride, w.Z, gi, gi.th));
  if (U) {
    gi.u = gi.th + per;
    TIMED(c, s, C_MISC, 0, launch_split_gate(s, d, c->po, U, tstride, w.Z, gi, gi.u));
  }
  w.gimg = gi;
  w.gimg_src = theta;
  w.gimg_u_src = U;
  return SMAML_OK;
}

// Pre-split images of theta's BPTT weights for this backward (launch_split_bwd) when the small-grid
// BPTT steps will read them (small_kw 2, batch-1 sizes); like the gate images, re-split every call.
int prep_bwd_images(smaml_ctx* c, hipStream_t s, const float* theta, int64_t tstride) {
  const Dims& d = c->d;
  Work& w = c->w;
  w.bimg = BwdImgs{};
  w.bimg_src = nullptr;
  if (c->kn.small_kw != 2 || !small_kw_ok(d, w) || (int64_t)w.Z * w.M > c->kn.wgrad_group_max_rows) return SMAML_OK;
  BwdImgs bi{};
  // no room: the BPTT steps load and split the f32 weights themselves
  if (c->bimg_buf.grow(bwd_img_bytes(d, &bi) * w.Z) != hipSuccess) return SMAML_OK;
  bi.th = c->bimg_buf.as<char>();
  TIMED(c, s, C_MISC, 0, launch_split_bwd(s, d, c->po, theta, tstride, w.Z, bi));
  w.bimg = bi;
  w.bimg_src = theta;
  return SMAML_OK;
}

// Layer 0's input projection of a step whose every task reads B consecutive windows, once per distinct
// stream row (kernels.h XgDedup, k_xg_dedup): the XG table of theta (want_xg) and / or of the sweep's
// tangent direction U, into w.xgd. Returns whether the tables were formed (no room, dropout, a batch of
// one or the option off: the gate kernels form the projection in their own K loops).
bool prep_xg_dedup(smaml_ctx* c, hipStream_t s, bool consec, const float* theta, const float* U, int64_t tstride,
                   bool want_xg) {
  const Dims& d = c->d;
  Work& w = c->w;
  w.xgd = XgDedup{};
  if (!consec || !c->kn.xg_dedup || w.B <= 1 || w.drop.gcn() || w.drop.lstm() || (!want_xg && !U)) return false;
  const int64_t per = xg_dedup_rows(w.B, d.T, d.N) * 4 * d.H;
  float* dst = xgd_scratch(c, per * w.Z * ((want_xg ? 1 : 0) + (U ? 1 : 0)));
  if (!dst) return false;
  XgDedup xd{};
  xd.zstride = per;
  xd.N = d.N;
  w.xgd = xd;  // (zstride read by the launcher)
  const double fl = 2.0 * w.Z * xg_dedup_rows(w.B, d.T, d.N) * 4 * d.H * c->po.lay[0].cin;
  if (want_xg) {
    const bool img = w.gimg.th && w.gimg_src == theta;
    TIMED(c, s, C_XG, fl,
          launch_xg_dedup(s, d, w, theta, tstride, c->po, img ? w.gimg.th : nullptr, w.gimg.tstride,
                          w.gimg.off[0][0], dst));
    xd.xg = dst;
    xd.src = theta;
    dst += per * w.Z;
  }
  if (U) {
    const bool img = w.gimg.u && w.gimg_u_src == U;
    TIMED(c, s, C_XG, fl,
          launch_xg_dedup(s, d, w, U, tstride, c->po, img ? w.gimg.u : nullptr, w.gimg.tstride, w.gimg.off[0][0],
                          dst));
    xd.rxg = dst;
    xd.u_src = U;
  }
  w.xgd = xd;
  return true;
}

// LSTM forward over all layers and time steps from w.F (anti-diagonal wavefront). consec: every task
// of this step reads B consecutive windows (layer 0's projection may then run once per stream row).
int run_lstm(smaml_ctx* c, hipStream_t s, const float* theta, int64_t tstride, bool consec = false) {
  const Dims& d = c->d;
  Work& w = c->w;
  TRY(prep_gate_images(c, s, theta, tstride));
  // big-tile steps (the meta-step's batches): the XG table when every layer-0 diagonal runs big tiles
  bool xgd_ok = consec;
  for (int diag = 0; xgd_ok && diag < d.T; ++diag) xgd_ok = fwd_wave_big(d, w, c->po, diag);
  const bool use_xgd = xgd_ok && prep_xg_dedup(c, s, true, theta, nullptr, tstride, true);
  if (w.fcompact && !use_xgd) return fail(SMAML_ESTATE, "compact features without the layer-0 projection table");
  // Batch-1 sizes (the small-grid steps): layer 0's input projection F . W_ih0^T does not depend on the
  // recurrence, so it runs for all T steps as one throughput-bound GEMM before the wavefront and the
  // layer-0 steps' latency-bound K loops cover only the recurrent segment (kernels_small.hip).
  w.xg = nullptr;
  w.xg_src = nullptr;
  // only the kw kernel reads the hoisted projection: hoist when every diagonal with a layer-0 step takes it
  bool hoist = small_kw_ok(d, w) && (int64_t)w.Z * w.M <= c->kn.wgrad_group_max_rows;
  for (int diag = 0; hoist && diag < d.T; ++diag) hoist = fwd_wave_kw(d, w, c->po, diag);
  if (hoist) {
    const int64_t per = (int64_t)d.T * w.M * 4 * d.H;
    // (no room: the layer-0 steps form the projection themselves)
    if (c->xg_buf.grow(per * w.Z * 4) == hipSuccess) {
      TIMED(c, s, C_XG, 2.0 * w.Z * d.T * w.M * 4 * d.H * d.Hc,
            launch_gemm_nt(s, w.F, (int64_t)d.T * w.M * d.Hc, d.T * w.M, d.Hc, theta + c->po.lay[0].wih, tstride,
                           4 * d.H, c->xg_buf.as<float>(), per, w.Z));
      w.xg = c->xg_buf.as<float>();
      w.xg_src = theta;
    }
  }
  // row chunks on side streams (fwd_chunks; big sizes only, where every diagonal runs the big tiles)
  const int nch = w.xg ? 1 : fwd_chunks(c);
  hipEvent_t wa = nullptr;
  if (nch > 1 && c->tm.on) (void)hipEventRecord(wa = c->tm.get(), s);
  if (nch > 1) TRY(fork_streams(c, s, nch));
  double wfl = 0.0;
  for (int diag = 0; diag < d.T + d.L - 1; ++diag) {
    FwdWave wv{};
    double fl = fwd_wave(d, w, c->po, diag, 0, false, wv);
    if ((w.xg && fwd_wave_kw(d, w, c->po, diag)) || use_xgd)  // (the projection's flops are counted above)
      for (int q = 0; q < wv.n; ++q)
        if (wv.l[q] == 0) fl -= 2.0 * w.Z * w.M * 4 * d.H * wv.lo[q].cin;
    wfl += fl;
    if (nch > 1) {
      for (int ci = 0; ci < nch; ++ci)
        TIMED(c, c->cs[ci], C_FWD, fl / nch,
              launch_lstm_fwd_wave(c->cs[ci], d, chunk_work(w, ci), diag, theta, tstride, c->po, nullptr, ci, nch));
    } else {
      TIMED(c, s, C_FWD, fl, launch_lstm_fwd_wave(s, d, w, diag, theta, tstride, c->po, nullptr));
    }
  }
  if (nch > 1) {
    TRY(join_streams(c, s, nch));
    time_wall(c, s, wa, C_FWD_WALL, wfl);
  }
  w.xg = nullptr;
  w.xg_src = nullptr;
  w.xgd = XgDedup{};
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

// New graph / GCN parameters / tasks: every cached window is stale, but the slots stay allocated (a
// re-allocation can cost seconds when the driver has to clear released VRAM, see ad_prepare).
static void ad_cache_invalidate(smaml_ctx* c) {
  for (auto& a : c->ad) std::fill(a.valid.begin(), a.valid.end(), (uint8_t)0);
}

int run_forward(smaml_ctx* c, hipStream_t s, const float* theta, int64_t tstride, const float* const* xtab_dev,
                const float* const* first_tab = nullptr) {
  TRY(run_gcn(c, s, xtab_dev, first_tab));
  c->w.consec = first_tab != nullptr;  // (read by the backward of these activations)
  return run_lstm(c, s, theta, tstride, first_tab != nullptr);
}

int run_bptt(smaml_ctx* c, hipStream_t s, const float* theta, int64_t tstride, float* grad);

// Backward from dpred (already written by k_head_loss) into grad [Z][P].
int run_backward(smaml_ctx* c, hipStream_t s, const float* theta, int64_t tstride, float* grad) {
  const Dims& d = c->d;
  Work& w = c->w;
  const ParamOff& po = c->po;
  const int64_t TM = (int64_t)d.T * w.M;
  const int64_t lsz = (int64_t)w.Z * TM * d.H;
  // batch-1 sizes without LSTM dropout: dh_T comes from the head's weight-gradient launch
  const bool dh_fused = head_small(d, w.M) && !w.drop.lstm();
  if (!dh_fused) TIMED(c, s, C_HEAD_DH, 2.0 * w.Z * w.M * d.HfC * d.H, launch_head_dh(s, d, w, theta, tstride, po));
  int64_t hz = 0;
  const float* hT = head_input(d, w, false, &hz);  // h_T, or drop(h_T) under dropout
  if (head_small(d, w.M)) {
    TIMED(c, s, C_WGRAD, (dh_fused ? 4.0 : 2.0) * w.Z * w.M * d.HfC * d.H,
          launch_head_wgrad_small(s, d, w, w.dpred, hT, hz, grad, po.P, po.wo, po.bo, dh_fused ? theta : nullptr,
                                  tstride));
    return run_bptt(c, s, theta, tstride, grad);
  }
  timed_wgrad(c, s, 2.0 * w.Z * w.M * d.HfC * d.H, w.dpred, (int64_t)w.M * d.HfC, d.HfC, hT, hz, d.H, nullptr, 0, 0,
                     w.M, 0, grad, po.P, po.wo, -1, po.bo, -1);
  return run_bptt(c, s, theta, tstride, grad);
}

// BPTT + LSTM weight gradients from the top layer's dh_T in w.dH [Z][M][H].
int run_bptt(smaml_ctx* c, hipStream_t s, const float* theta, int64_t tstride, float* grad) {
  const Dims& d = c->d;
  Work& w = c->w;
  const ParamOff& po = c->po;
  const int64_t TM = (int64_t)d.T * w.M;
  const int64_t lsz = (int64_t)w.Z * TM * d.H;
  // BPTT as reverse anti-diagonals; layer l's weight gradient as soon as its t = 0 step is done,
  // or, for small grids (batch-1 adaptation), all layers' in one launch after the sweep
  const bool grouped = (int64_t)w.Z * w.M <= c->kn.wgrad_group_max_rows;
  TRY(prep_bwd_images(c, s, theta, tstride));
  WgradPlan plans[MAX_LAYERS];
  double gfl = 0.0;
  auto layer_wgrad = [&](int l) {
    const LayerOff& lo = po.lay[l];
    const float* X = l == 0 ? w.F : w.Hs + (int64_t)(l - 1) * lsz;
    if (grouped) {
      WgradPlan& p = plans[l];
      plan_wgrad(w, w.dG + (int64_t)l * lsz * 4, TM * 4 * d.H, 4 * d.H, X, TM * lo.cin, lo.cin,
                 w.Hs + (int64_t)l * lsz, TM * d.H, d.H, TM, w.M, grad, po.P, lo.wih, lo.whh, lo.bih, lo.bhh, true,
                 false, p, true);
      p.drop = w.drop;
      p.drop_layer = l - 1;
      gfl += 2.0 * w.Z * TM * 4 * d.H * (lo.cin + d.H);
      return;
    }
    if (l == 0 && wgrad_dedup_ok(c) && timed_wgrad_ih0_dedup(c, s, w.dG, grad)) {
      // W_hh0 and the bias over every row (h_{t-1} differs per window): [0 | h_{t-1}], no input columns
      timed_wgrad(c, s, 2.0 * w.Z * TM * 4 * d.H * d.H, w.dG, TM * 4 * d.H, 4 * d.H, nullptr, 0, 0, w.Hs, TM * d.H,
                  d.H, TM, w.M, grad, po.P, -1, lo.whh, lo.bih, lo.bhh, true, false, -1);
      return;
    }
    timed_wgrad(c, s, 2.0 * w.Z * TM * 4 * d.H * (lo.cin + d.H), w.dG + (int64_t)l * lsz * 4, TM * 4 * d.H, 4 * d.H, X,
                TM * lo.cin, lo.cin, w.Hs + (int64_t)l * lsz, TM * d.H, d.H, TM, w.M, grad, po.P, lo.wih, lo.whh,
                lo.bih, lo.bhh, true, false, l - 1);
  };
  // after a chunked sweep: layers L-1 .. 0 on the caller's stream
  auto after_sweep_wgrads = [&]() {
    for (int l = d.L - 1; l >= 0; --l) layer_wgrad(l);
  };
  // row chunks on side streams (knob bptt_streams): every diagonal's big-tile launch split by rows, the
  // weight gradients after the sweep on the caller's stream
  // (chunked only where a full diagonal runs the big tiles anyway: tile-forcing knobs keep their meaning)
  const int nch = grouped || !bwd_wave_big(d, w, po, std::min(d.L, d.T) - 1) ? 1 : c->kn.bptt_streams;
  hipEvent_t wa = nullptr;
  if (nch > 1 && c->tm.on) (void)hipEventRecord(wa = c->tm.get(), s);
  if (nch > 1) TRY(fork_streams(c, s, nch));
  double wfl = 0.0;
  for (int e = 0; e < d.T + d.L - 1; ++e) {
    BwdWave wv{};
    const double fl = bwd_wave(d, w, po, e, 0, false, wv);
    wfl += fl;
    if (nch > 1) {
      for (int ci = 0; ci < nch; ++ci)
        TIMED(c, c->cs[ci], C_BWD, fl / nch, launch_lstm_bwd_wave(c->cs[ci], d, chunk_work(w, ci), e, theta, tstride, po, ci, nch));
    } else {
      TIMED(c, s, C_BWD, fl, launch_lstm_bwd_wave(s, d, w, e, theta, tstride, po));
    }
    const int l = d.L - 1 - (e - (d.T - 1));
    if (e < d.T - 1 || l < 0) continue;
    if (nch <= 1) layer_wgrad(l);
  }
  if (nch > 1) {
    TRY(join_streams(c, s, nch));
    time_wall(c, s, wa, C_BWD_WALL, wfl);
    after_sweep_wgrads();
  }
  if (grouped) TIMED(c, s, C_WGRAD, gfl, launch_wgrad_multi(s, w, plans, d.L, c->kn.wgrad_group_wgs));
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

// Primal recompute + tangent along U (second-order sweep), GCN features recomputed.
// gcn_cached: w.F is the step's so_F slot, written by the inner loop's GCN in the layout fcompact_rec
// recorded then (not re-derived: f_compact_ok allocates, so a later call could decide differently).
int run_forward_dual(smaml_ctx* c, hipStream_t s, const float* theta, const float* U, int64_t tstride,
                     const float* const* xtab_dev, bool gcn_cached, const float* const* first_tab, int fcompact_rec) {
  const Dims& d = c->d;
  Work& w = c->w;
  if (!gcn_cached) TRY(run_gcn(c, s, xtab_dev, first_tab));
  else w.fcompact = fcompact_rec;
  w.consec = first_tab != nullptr;
  TRY(prep_gate_images(c, s, theta, tstride, U));
  // layer 0's tangent projection F U_ih0^T (and, unless the primal is kept, F W_ih0^T) once per stream row
  const bool use_xgd = prep_xg_dedup(c, s, first_tab != nullptr, theta, U, tstride, !w.primal_kept);
  if (w.fcompact && !use_xgd) return fail(SMAML_ESTATE, "compact features without the layer-0 projection tables");
  const int nch = fwd_chunks(c);  // (row chunks on side streams)
  hipEvent_t wa = nullptr;
  if (nch > 1 && c->tm.on) (void)hipEventRecord(wa = c->tm.get(), s);
  if (nch > 1) TRY(fork_streams(c, s, nch));
  double wfl = 0.0;
  for (int diag = 0; diag < d.T + d.L - 1; ++diag) {
    FwdWave wv{};
    double fl = fwd_wave(d, w, c->po, diag, 0, true, wv);
    if (w.primal_kept) fl -= fwd_wave(d, w, c->po, diag, 0, false, wv);  // tangent pass only
    if (use_xgd)  // (counted in C_XG)
      for (int q = 0; q < wv.n; ++q)
        if (wv.l[q] == 0) fl -= (w.primal_kept ? 1.0 : 2.0) * 2.0 * w.Z * w.M * 4 * d.H * wv.lo[q].cin;
    wfl += fl;
    if (nch > 1) {
      for (int ci = 0; ci < nch; ++ci)
        TIMED(c, c->cs[ci], C_FWD_DUAL, fl / nch,
              launch_lstm_fwd_dual_wave(c->cs[ci], d, chunk_work(w, ci), diag, theta, U, tstride, c->po, nullptr, ci, nch));
    } else {
      TIMED(c, s, C_FWD_DUAL, fl, launch_lstm_fwd_dual_wave(s, d, w, diag, theta, U, tstride, c->po, nullptr));
    }
  }
  if (nch > 1) {
    TRY(join_streams(c, s, nch));
    time_wall(c, s, wa, C_FWD_DUAL_WALL, wfl);
  }
  w.xgd = XgDedup{};
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

// Tangent of the backward pass: HU[z] = H_z U[z] (primal weight grads are not formed).
int run_backward_dual(smaml_ctx* c, hipStream_t s, const float* theta, const float* U, int64_t tstride, float* HU) {
  const Dims& d = c->d;
  Work& w = c->w;
  const ParamOff& po = c->po;
  const int64_t TM = (int64_t)d.T * w.M;
  const int64_t lsz = (int64_t)w.Z * TM * d.H;
  TIMED(c, s, C_HEAD_DH, 3.0 * 2.0 * w.Z * w.M * d.HfC * d.H, launch_head_dh_dual(s, d, w, theta, U, tstride, po));
  int64_t hz = 0;
  const float* hT = head_input(d, w, false, &hz);
  const float* RhT = head_input(d, w, true, &hz);
  timed_wgrad(c, s, 2.0 * w.Z * w.M * d.HfC * d.H, w.Rdpred, (int64_t)w.M * d.HfC, d.HfC, hT, hz, d.H, nullptr, 0, 0,
                     w.M, 0, HU, po.P, po.wo, -1, po.bo, -1, true, false);
  timed_wgrad(c, s, 2.0 * w.Z * w.M * d.HfC * d.H, w.dpred, (int64_t)w.M * d.HfC, d.HfC, RhT, hz, d.H, nullptr, 0, 0,
                     w.M, 0, HU, po.P, po.wo, -1, po.bo, -1, false, true);
  auto layer_wgrad = [&](int l) {
    const LayerOff& lo = po.lay[l];
    const float* X = l == 0 ? w.F : w.Hs + (int64_t)(l - 1) * lsz;
    const float* RX = l == 0 ? nullptr : w.RHs + (int64_t)(l - 1) * lsz;
    const float* dGl = w.dG + (int64_t)l * lsz * 4;
    const float* RdGl = w.RGs + (int64_t)l * lsz * 4;
    if (l == 0 && wgrad_dedup_ok(c) && timed_wgrad_ih0_dedup(c, s, RdGl, HU)) {
      // R(dW_ih0) = R(dG0)^T F (R x = 0 at layer 0) over distinct stream rows above; R(dW_hh0) =
      // R(dG0)^T h + dG0^T R h and R(db) as one paired launch over every row
      const double flp = 2.0 * 2.0 * w.Z * TM * 4 * d.H * d.H;
      if (!(c->kn.wgrad_pair && timed_wgrad_pair(c, s, flp, RdGl, dGl, TM * 4 * d.H, 4 * d.H, nullptr, nullptr, 0, 0,
                                                 w.Hs, w.RHs, TM * d.H, d.H, TM, w.M, HU, po.P, -1, lo.whh, lo.bih,
                                                 lo.bhh, -1))) {
        timed_wgrad(c, s, flp / 2, RdGl, TM * 4 * d.H, 4 * d.H, nullptr, 0, 0, w.Hs, TM * d.H, d.H, TM, w.M, HU, po.P,
                    -1, lo.whh, lo.bih, lo.bhh, true, false, -1);
        timed_wgrad(c, s, flp / 2, dGl, TM * 4 * d.H, 4 * d.H, nullptr, 0, 0, w.RHs, TM * d.H, d.H, TM, w.M, HU, po.P,
                    -1, lo.whh, lo.bih, lo.bhh, false, true, -1);
      }
      return;
    }
    if (l > 0 && c->kn.wgrad_pair &&  // both passes 4H x (cin + H): one launch
        timed_wgrad_pair(c, s, 2.0 * 2.0 * w.Z * TM * 4 * d.H * (lo.cin + d.H), RdGl, dGl, TM * 4 * d.H, 4 * d.H, X,
                         RX, TM * lo.cin, lo.cin, w.Hs + (int64_t)l * lsz, w.RHs + (int64_t)l * lsz, TM * d.H, d.H,
                         TM, w.M, HU, po.P, lo.wih, lo.whh, lo.bih, lo.bhh, l - 1))
      return;
    timed_wgrad(c, s, 2.0 * w.Z * TM * 4 * d.H * (lo.cin + d.H), RdGl, TM * 4 * d.H, 4 * d.H, X, TM * lo.cin, lo.cin,
                w.Hs + (int64_t)l * lsz, TM * d.H, d.H, TM, w.M, HU, po.P, lo.wih, lo.whh, lo.bih, lo.bhh, true, false,
                l - 1);
    timed_wgrad(c, s, 2.0 * w.Z * TM * 4 * d.H * ((l > 0 ? lo.cin : 0) + d.H), dGl, TM * 4 * d.H, 4 * d.H, RX,
                TM * lo.cin, l > 0 ? lo.cin : 0, w.RHs + (int64_t)l * lsz, TM * d.H, d.H, TM, w.M, HU, po.P, lo.wih,
                lo.whh, lo.bih, lo.bhh, false, true, l - 1);
  };
  // after a chunked sweep: layers L-1 .. 0 on the caller's stream
  auto after_sweep_wgrads = [&]() {
    for (int l = d.L - 1; l >= 0; --l) layer_wgrad(l);
  };
  const int nch = (int64_t)w.Z * w.M <= c->kn.wgrad_group_max_rows || !bwd_dual_wave_big(d, w, po, std::min(d.L, d.T) - 1)
                      ? 1
                      : c->kn.bptt_streams;
  hipEvent_t wa = nullptr;
  if (nch > 1 && c->tm.on) (void)hipEventRecord(wa = c->tm.get(), s);
  if (nch > 1) TRY(fork_streams(c, s, nch));
  double wfl = 0.0;
  for (int e = 0; e < d.T + d.L - 1; ++e) {
    BwdWave wv{};
    const double fl = bwd_wave(d, w, po, e, 0, true, wv) * (w.primal_kept ? 2.0 / 3.0 : 1.0);
    wfl += fl;
    if (nch > 1) {
      for (int ci = 0; ci < nch; ++ci)
        TIMED(c, c->cs[ci], C_BWD_DUAL, fl / nch,
              launch_lstm_bwd_dual_wave(c->cs[ci], d, chunk_work(w, ci), e, theta, U, tstride, po, ci, nch));
    } else {
      TIMED(c, s, C_BWD_DUAL, fl, launch_lstm_bwd_dual_wave(s, d, w, e, theta, U, tstride, po));
    }
    const int l = d.L - 1 - (e - (d.T - 1));
    if (e < d.T - 1 || l < 0) continue;
    if (nch <= 1) layer_wgrad(l);
  }
  if (nch > 1) {
    TRY(join_streams(c, s, nch));
    time_wall(c, s, wa, C_BWD_DUAL_WALL, wfl);
    after_sweep_wgrads();
  }
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

bool graph_set(const smaml_ctx* c) { return c->graph_form != 0; }

int require_ready(smaml_ctx* c) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  if (!graph_set(c)) return fail(SMAML_ESTATE, "smaml_set_graph not called");
  if (!c->gcn) return fail(SMAML_ESTATE, "smaml_set_gcn_params not called");
  return SMAML_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the bookkeeping kernels' grid-barrier state (zeroed once; self-resetting, see kernels.h GridBar)
int ensure_bar(smaml_ctx* c) {
  if (c->bar.ptr) return SMAML_OK;
  int khz = 0;
  HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
  c->wall_khz = khz > 0 ? (uint64_t)khz : 100000;
  HIP_TRY(hipHostMalloc((void**)&c->bar_err_host, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
  *(volatile int*)c->bar_err_host = 0;
  HIP_TRY(hipHostGetDevicePointer((void**)&c->bar_err_dev, c->bar_err_host, 0));
  HIP_TRY(c->bar.grow(4 * sizeof(unsigned)));
  HIP_TRY(hipMemset(c->bar.ptr, 0, 4 * sizeof(unsigned)));
  HIP_TRY(hipDeviceSynchronize());
  return SMAML_OK;
}

BarPlan bar_plan(const smaml_ctx* c) {
  BarPlan bp{};
  bp.gb.w = c->bar.as<unsigned>();
  bp.gb.host_err = c->bar_err_dev;
  bp.gb.timeout = (uint64_t)c->bar_timeout_us * c->wall_khz / 1000;
  bp.fused = c->bar_fused;
  bp.oversize = c->bar_oversize;
  return bp;
}

// A grid-barrier wait that timed out (kernels.h grid_barrier) raised the pinned flag: drain the device,
// reset the barrier state and report it. No host sync unless the flag is up.
int check_device_error(smaml_ctx* c) {
  if (!c->bar_err_host || *(volatile int*)c->bar_err_host == 0) return SMAML_OK;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(c->bar.ptr, 0, 4 * sizeof(unsigned)));
  HIP_TRY(hipDeviceSynchronize());
  *(volatile int*)c->bar_err_host = 0;
  return fail(SMAML_EHIP,
              "a grid-barrier kernel (k_inner_sgd / k_sweep_update) timed out waiting for its grid: the grid was "
              "not co-resident (another process holding the GPU, or the barrier_oversize debug knob); its "
              "results are invalid");
}

// Backward of z = A_hat x W^T + b over `rows` rows given dz [rows][cout] (smaml_gcn_conv_backward, and every
// layer of smaml_backward_base). The rows are samples of rps rows each; each sample's first ng rows
// aggregate over the graph (ng = 0: A_hat = I), the rest see only their self loop (F3). dx [rows][cin]
// (optional) = A_hat^T (dz W); grad (optional): dW (cout x cin, row-major) at off_w and db (cout) at off_b,
// summed over all rows, overwritten. Scratch: c->bw_scratch (grown here; grow it before the first launch of
// a call that must not stall mid-way). Fixed-order sums.
int gcn_conv_bwd(smaml_ctx* c, hipStream_t s, const float* x, int rows, int rps, int cin, const float* weight, int cout,
                 const float* dz, int ng, float* dx, float* grad, int64_t off_w, int64_t off_b) {
  const int64_t half = (int64_t)rows * std::max(cin, cout);
  HIP_TRY(c->bw_scratch.grow(2 * half * 4));
  float* t0 = c->bw_scratch.as<float>();
  float* t1 = t0 + half;
  if (grad) {
    // dW = dz^T (A_hat x), db = sum_rows dz: the split-K weight-gradient GEMM with its bias column
    const float* ax = x;
    if (ng > 0) {
      // A_hat x through the ELL, or through A_hat's CSR (k_gather_rows's CSR sum, the one A_hat^T takes below)
      const GraphView gv = graph_view(c);
      if (gv.form == 2) {
        launch_gather_rows(s, x, t0, rows, cin, ng, nullptr, nullptr, gv.csr_p, gv.csr_c, gv.csr_v, rps);
        ++c->graph_stats[4];
      } else {
        launch_gather_rows(s, x, t0, rows, cin, ng, gv.ell_c, gv.ell_v, nullptr, nullptr, nullptr, rps);
      }
      ax = t0;
    }
    Work w = c->w;
    w.Z = 1;
    w.drop = Drop{};
    w.kn = c->kn;
    launch_wgrad(s, c->d, w, dz, 0, cout, ax, 0, cin, nullptr, 0, 0, rows, 0, grad, 0, off_w, off_w, off_b, -1, true,
                 false);
  }
  if (dx) {
    // dx = A_hat^T (dz W): the rows past the graph's nodes see only their self loop
    if (ng > 0) {
      launch_gemm_nn_plain(s, dz, rows, cout, weight, cin, t1);
      launch_gather_rows(s, t1, dx, rows, cin, ng, nullptr, nullptr, c->tr_p.as<int32_t>(), c->tr_c.as<int32_t>(),
                         c->tr_v.as<float>(), rps);
      if (c->graph_form == 2) ++c->graph_stats[4];
    } else {
      launch_gemm_nn_plain(s, dz, rows, cout, weight, cin, dx);
    }
  }
  return SMAML_OK;
}

// The GCN backward, conv4 -> conv1, over `rows` rows (samples of rps rows) from dZ4 in g (smaml_backward_base and
// the step that trains the base). Per layer l: dW, db of conv l+1 into grad at the layer's offsets (grad null:
// none), then -- unless it is conv1 and its input gradient is not wanted -- dz . W, the A_hat^T gather, the mask
// of the dropout (replayed) and the ReLU after conv l (its kept output h[l-1]; conv1's input has none), and
// g <-> gn. x0: conv1's input [rows][Cin0]. dz_top: k_gcn_dz's scratch, which selects the one-launch form of
// the layer-to-layer gradient (null: GEMM + gather + mask; bitwise the same). stats (optional): [3] += k_gcn_dz
// launches, [4] += launches of the composed form. cat: the timing category of the layer-to-layer launches. On
// return g holds the last gradient written (conv1's input gradient [rows][Cin0] when want_dx0). ng: the rows of
// each sample that aggregate over the graph (default N; 0: a neighbour-less block, A_hat = I, on the composed
// form: the stream rows past t = 0 of smaml_meta_step_base's distinct-row stage).
int gcn_backward_chain(smaml_ctx* c, hipStream_t s, const float* x0, float* const h[3], float*& g, float*& gn, int rows,
                       int rps, const float* gcn, float* grad, bool want_dx0, float* dz_top, int64_t* stats, int cat,
                       int ng = -1) {
  const Dims& d = c->d;
  if (ng < 0) ng = d.N;
  if (ng == 0) dz_top = nullptr;  // (k_gcn_dz gathers every sample's first N rows)
  const float sc = c->w.drop.gcn() ? c->w.drop.sc_gcn : 1.f;
  for (int l = 3; l >= 0; --l) {
    const float* x = l == 0 ? x0 : h[l - 1];
    const float* W = gcn + c->go.w[l];
    const int cin = c->go.cin[l];
    if (grad) TRY(gcn_conv_bwd(c, s, x, rows, rps, cin, W, d.Hc, g, ng, nullptr, grad, c->go.w[l], c->go.b[l]));
    if (l == 0 && !want_dx0) break;
    if (l > 0 && dz_top) {
      TIMED(c, s, cat, 2.0 * rows * d.Hc * cin,
            launch_gcn_dz(s, g, rows, d.Hc, W, cin, h[l - 1], sc, rps, d.N, c->tr_p.as<int32_t>(), c->tr_c.as<int32_t>(),
                          c->tr_v.as<float>(), dz_top, gn));
      if (stats) stats[3] += 1;
      if (c->graph_form == 2) ++c->graph_stats[4];
    } else {
      TIMED(c, s, cat, 2.0 * rows * d.Hc * cin, {
        TRY(gcn_conv_bwd(c, s, x, rows, rps, cin, W, d.Hc, g, ng, gn, nullptr, 0, 0));
        if (l > 0) launch_drop_relu_grad(s, gn, h[l - 1], (int64_t)rows * d.Hc, sc);
      });
      if (stats) stats[4] += l > 0 ? 3 : 2;
    }
    std::swap(g, gn);
  }
  return SMAML_OK;
}

// ---- the forecast family: smaml_forecast, _ensemble, _rollout, _rollout_ensemble --------------------------
// Inference on buffers of their own. Every entry point is forecast_check, its buffers and pointer table, then
// forecast_run over its pass function; every pass function is a sequence of the stages below.

// One call as its entry point received it.
struct ForecastCall {
  const char* name = nullptr;       // the entry point, for messages
  const char* no_output = nullptr;  // what the message says of a call whose output pointers are all NULL
  bool any_output = false;
  const float* theta = nullptr;
  const int32_t* list = nullptr;    // window starts; rollouts: origins
  int n = 0, batch = 0, task = 0;
  bool score = false;               // skill / scores asked for
  const float* scale_host = nullptr;
  bool rollout = false;
  int cycles = 0, gap = 0;
  bool ens = false;
  int members = 0;
  float p_gcn = 0.f, p_lstm = 0.f;
  uint32_t seed = 0;
};

constexpr int RENS_MAX_CYCLES = 1024;  // drop_site gives `step` 16 bits (step << 8 below kind << 24): 64 j + e < 2^16

// rows of an origin's private sequence: its window, then the Hf + 1 rows every cycle but the last appends
int64_t roll_seq_rows(const Dims& d, int R) { return d.T + (int64_t)(R - 1) * (d.Hf + 1); }

// The argument checks (they need no context and run without a device too), the state checks, then every window
// or origin against its stream: its input rows must fit and, when scoring, so must the last targets, Hf + 1
// rows on. Last the device.
int forecast_check(smaml_ctx* c, const ForecastCall& a) {
  const std::string fn = std::string(a.name) + ": ";
  if (!a.any_output) return fail(SMAML_EINVAL, fn + a.no_output);
  if (a.n <= 0 || a.batch <= 0 || !a.list)
    return fail(SMAML_EINVAL, fn + (a.rollout ? "norig" : "nwin") + " and batch must be positive");
  if (a.ens && (a.members < 1 || a.members > 64))
    return fail(SMAML_EINVAL, fn + "members must be in 1..64, got " + std::to_string(a.members));
  if (a.rollout && !a.ens && a.cycles <= 0) return fail(SMAML_EINVAL, fn + "cycles must be positive");
  if (a.rollout && a.ens && (a.cycles < 1 || a.cycles > RENS_MAX_CYCLES))
    return fail(SMAML_EINVAL, fn + "cycles must be in 1.." + std::to_string(RENS_MAX_CYCLES) +
                                  " (the mask site's step 64 j + e has 16 bits), got " + std::to_string(a.cycles));
  if (a.ens && (!(a.p_gcn >= 0.f && a.p_gcn < 1.f) || !(a.p_lstm >= 0.f && a.p_lstm < 1.f)))
    return fail(SMAML_EINVAL, fn + "dropout probabilities must be in [0, 1)");
  if (a.rollout && a.gap != 0 && a.gap != 1)
    return fail(SMAML_EINVAL, fn + "gap must be 0 (persistence) or 1 (midpoint), got " + std::to_string(a.gap));
  TRY(require_ready(c));
  TRY(check_lstm_dims(c->dims, a.name));
  if (c->feats.empty()) return fail(SMAML_ESTATE, "smaml_set_tasks not called");
  if (!a.theta || !aligned16(a.theta)) return fail(SMAML_EINVAL, fn + "theta must be a 16-byte aligned device pointer");
  if (a.task < 0 || a.task >= (int)c->feats.size()) return fail(SMAML_EINVAL, fn + "task out of range");
  const Dims& d = c->d;
  if ((int64_t)d.T * std::min(a.batch, a.n) * d.N * 4 * d.H >= (a.rollout ? 1ll << 30 : 1ll << 31))
    return fail(SMAML_EINVAL,
                std::string("batch too large: T*B*N*4H must stay below ") + (a.rollout ? "2^30" : "2^31"));
  const int64_t tt = c->t_total[a.task];
  const int64_t need_in = a.rollout ? roll_seq_rows(d, a.cycles) : d.T, need_sc = need_in + d.Hf + 1;
  for (int i = 0; i < a.n; ++i) {
    const int64_t o = a.list[i];
    const bool fits = o >= 0 && o + need_in <= tt;
    if (fits && !(a.score && o + need_sc > tt)) continue;
    std::string m = fn + (a.rollout ? "origin " : "window ") + std::to_string(i) + " (start " + std::to_string(o);
    if (a.rollout)
      m += (fits ? ") has no targets for " : ") does not fit ") + std::to_string(a.cycles) + " cycles in";
    else
      m += fits ? ") has no targets in" : ") does not fit";
    return fail(SMAML_EINVAL, m + " the stream of " + std::to_string(tt) + " steps");
  }
  TRY(ensure_device(c));
  TRY(check_device_error(c));
  return SMAML_OK;
}

// The pointer table of a call over windows: entry i = window i's first stream row.
std::vector<const float*> window_ptrs(const smaml_ctx* c, const ForecastCall& a) {
  std::vector<const float*> ptrs(a.n);
  for (int i = 0; i < a.n; ++i) ptrs[i] = c->feats[a.task] + (int64_t)a.list[i] * c->d.N * c->d.Cin0;
  return ptrs;
}

// whether a pass's B windows start at consecutive stream rows (w[b] = w[0] + b; a single window does not count)
bool windows_consec(const int32_t* w, int B) {
  bool consec = B > 1;
  for (int b = 1; b < B && consec; ++b) consec = w[b] == w[0] + b;
  return consec;
}

// Uploads the scale (when scoring with one) and the pointer table, then body(done, B, scale_dev) per pass of at
// most a.batch entries. The training state stays as it is: the family never touches the arena, and the
// workspace view (with the activations a pending smaml_backward / smaml_lstm_backward will consume) is put
// back on every path.
template <class Body>
int forecast_run(smaml_ctx* c, hipStream_t s, const ForecastCall& a, const std::vector<const float*>& ptrs, Body body) {
  const Work saved = c->w;
  const int act = c->act_B;
  auto run = [&]() -> int {
    const float* scale_dev = nullptr;
    if (a.score && a.scale_host) {
      HIP_TRY(c->fc_scale.grow((int64_t)c->d.C * 4));
      TRY(c->stage.upload(s, c->fc_scale.ptr, a.scale_host, (int64_t)c->d.C * 4));
      scale_dev = c->fc_scale.as<float>();
    }
    TRY(upload_xtab(c, s, ptrs.data(), (int64_t)ptrs.size()));
    for (int64_t done = 0; done < a.n; done += a.batch)
      TRY(body(done, (int)std::min<int64_t>(a.batch, a.n - done), scale_dev));
    return SMAML_OK;
  };
  const int rc = run();
  c->w = saved;
  c->act_B = act;
  return rc;
}

// -- stages --
// c->w for a pass of B windows or origins, on the forecast's buffers
void forecast_work(smaml_ctx* c, int B) {
  Work w{};
  w.Z = 1;
  w.B = B;
  w.M = B * c->d.N;
  w.F = c->fc_F.as<float>();
  w.gcnA = c->fc_gcnA.as<float>();
  w.gcnB = c->fc_gcnB.as<float>();
  w.vcount = c->vcount;
  w.kn = c->kn;
  c->w = w;
}

// Whether a forecast pass of consecutive windows stores its GCN features compact (the distinct stream
// rows only, XgDedup order). The forecast's only reader of F is layer 0's gate step -- every diagonal on
// the big tiles (k_lstm_fwd_infer has no other form) and nothing differentiates -- so unlike f_compact_ok
// neither the weight-gradient path nor the tile choice enters: it takes the GCN and the projection once
// per distinct row (the options of the training step) and the table they go through.
bool forecast_compact_ok(const smaml_ctx* c, bool consec, int B, bool have_xg) {
  const Knobs& kn = c->kn;
  return consec && B > 1 && kn.f_compact && kn.gcn_dedup && kn.xg_dedup && have_xg;
}

// How a pass of B windows shares its GCN features: layer 0's projection per distinct stream row (have_xg;
// grows fc_xg), F compact, and the rows of F (frows) and of the GCN scratch (grows: the t = 0 blocks on the
// fused path; else every row, or (per-layer dedup) each task's B + T - 1 stream rows).
struct FeatPlan {
  bool have_xg = false, compact = false;
  int64_t xrows = 0, frows = 0, grows = 0;
};

FeatPlan feat_plan(smaml_ctx* c, int B, bool consec) {
  const Dims& d = c->d;
  const Knobs& kn = c->kn;
  const int64_t M = (int64_t)B * d.N;
  FeatPlan f;
  f.xrows = xg_dedup_rows(B, d.T, d.N);
  f.have_xg = consec && kn.xg_dedup && B > 1 && c->fc_xg.grow(f.xrows * 4 * d.H * 4) == hipSuccess;
  f.compact = forecast_compact_ok(c, consec, B, f.have_xg);
  f.frows = f.compact ? f.xrows : d.T * M;
  f.grows = gcn_mlp_supported(d) && kn.gcn_fused    ? M
            : consec && kn.gcn_dedup && B > 1       ? std::max<int64_t>((int64_t)(B + d.T - 1) * d.N, M)
                                                    : d.T * M;
  return f;
}

// The features every row of the pass reads, once: the GCN into c->w.F, the gate images and, with have_xg, layer
// 0's projection of the distinct stream rows into fc_xg (c->w.xgd).
int shared_features(smaml_ctx* c, hipStream_t s, const float* theta, const float* const* xt, bool consec,
                    const FeatPlan& f) {
  const Dims& d = c->d;
  TRY(run_gcn(c, s, xt, consec ? xt : nullptr, f.compact ? 1 : 0));
  TRY(prep_gate_images(c, s, theta, 0));
  Work& cw = c->w;
  if (f.have_xg) {
    XgDedup xd{};
    xd.zstride = f.xrows * 4 * d.H;
    xd.N = d.N;
    cw.xgd = xd;  // (zstride read by the launcher)
    float* dst = c->fc_xg.as<float>();
    const bool img = cw.gimg.th && cw.gimg_src == theta;
    TIMED(c, s, C_XG, 2.0 * f.xrows * 4 * d.H * c->po.lay[0].cin,
          launch_xg_dedup(s, d, cw, theta, 0, c->po, img ? cw.gimg.th : nullptr, cw.gimg.tstride, cw.gimg.off[0][0],
                          dst));
    xd.xg = dst;
    xd.src = theta;
    cw.xgd = xd;
  }
  return SMAML_OK;
}

// The inference wavefront of c->w on rings [L][2][1][M][H] and the head into pred [M][HfC]. (Layer 0's
// projection, when c->w.xgd tables it, is counted in C_XG.)
void infer_waves(smaml_ctx* c, hipStream_t s, const float* theta, float* ringH, float* ringC, float* pred) {
  const Dims& d = c->d;
  const Work& cw = c->w;
  const int M = cw.M;
  for (int diag = 0; diag < d.T + d.L - 1; ++diag) {
    FwdWave wv{};
    double fl = fwd_wave(d, cw, c->po, diag, 0, false, wv);
    if (cw.xgd.xg)
      for (int q = 0; q < wv.n; ++q)
        if (wv.l[q] == 0) fl -= 2.0 * M * 4 * d.H * wv.lo[q].cin;
    TIMED(c, s, C_FWD, fl, launch_lstm_fwd_infer(s, d, cw, diag, theta, 0, c->po, ringH, ringC));
  }
  TIMED(c, s, C_HEAD, 2.0 * M * d.HfC * d.H,
        launch_head_pred(s, d, cw, infer_ring_hT(d, ringH, 1, M), (int64_t)M * d.H, theta, 0, c->po, pred));
}

// The same for g members in lockstep (grid z) under the masks of ed, member z's features fz floats past c->w.F
// (0: shared): the wavefront on rings [L][2][g][M][H], the kind-3 mask of every member's h_T, the head into
// pred [g][M][HfC]. Layer 0 counts once when ed.share0, and without its projection when tabled.
void infer_waves_drop(smaml_ctx* c, hipStream_t s, const float* theta, float* ringH, float* ringC, int g, int64_t fz,
                      const EnsDrop& ed, float* pred) {
  const Dims& d = c->d;
  const Work& cw = c->w;
  const int M = cw.M;
  for (int diag = 0; diag < d.T + d.L - 1; ++diag) {
    FwdWave wv{};
    double fl = 0.0;
    fwd_wave(d, cw, c->po, diag, 0, false, wv);
    for (int q = 0; q < wv.n; ++q) {
      const double k1 = (wv.l[q] == 0 && cw.xgd.xg ? 0 : wv.lo[q].cin) + (wv.t[q] > 0 ? d.H : 0);
      fl += 2.0 * (wv.l[q] == 0 && ed.share0 ? 1 : g) * M * 4 * d.H * k1;
    }
    TIMED(c, s, C_FWD, fl, launch_lstm_fwd_infer_drop(s, d, cw, diag, theta, c->po, ringH, ringC, g, fz, ed));
  }
  float* hT = const_cast<float*>(infer_ring_hT(d, ringH, g, M));
  if (ed.thr)
    TIMED(c, s, C_HEAD, 0,
          launch_ens_dropout(s, hT, (int64_t)M * d.H, g, ed.seed, 3, ed.e0, 0, ed.thr, ed.sc, (uint64_t)ed.row0 * d.H));
  Work hw = cw;
  hw.Z = g;
  TIMED(c, s, C_HEAD, 2.0 * g * M * d.HfC * d.H, launch_head_pred(s, d, hw, hT, (int64_t)M * d.H, theta, 0, c->po, pred));
}

// The masks of a call's LSTM dropout for the pass whose first entry is `done` of the call's n
EnsDrop ens_drop(const Dims& d, const ForecastCall& a, int64_t done) {
  EnsDrop ed{};
  ed.seed = a.seed;
  ed.thr = (uint32_t)std::lround((double)a.p_lstm * 16777216.0);
  ed.sc = 1.f / (1.f - a.p_lstm);
  ed.row0 = done * d.N;
  ed.Mtot = (int64_t)a.n * d.N;
  return ed;
}

// One member's STGCN features under its own masks, into dst [T][M][Hc]: conv k over the B samples of T N rows
// that start at tab[b] (the t = 0 rows with the graph), then the kind-1 mask of (step, layer k) at the call-wide
// element index base + the buffer's own linear index.
void member_gcn_masked(smaml_ctx* c, hipStream_t s, const float* const* tab, const ForecastCall& a, int step,
                       uint64_t base, float* dst) {
  const Dims& d = c->d;
  const Work& cw = c->w;
  const int B = cw.B, rps = d.T * d.N;
  const GraphView gv = graph_view(c);
  const uint32_t thr_gcn = (uint32_t)std::lround((double)a.p_gcn * 16777216.0);
  float* bufs[2] = {cw.gcnA, cw.gcnB};
  const float* from = nullptr;
  for (int k = 0; k < 4; ++k) {
    const bool last = k == 3;
    float* to = last ? dst : bufs[k & 1];
    TIMED(c, s, C_GCN, 2.0 * B * rps * c->go.cin[k] * d.Hc,
          launch_gcn_layer(s, d, k, B, B, k == 0 ? tab : nullptr, from, to, last, true, c->gcn + c->go.w[k],
                           c->gcn + c->go.b[k], c->go.cin[k], d.Hc, gv, rps, d.N, nullptr));
    if (!last)
      TIMED(c, s, C_GCN, 0,
            launch_ens_dropout(s, to, (int64_t)B * rps * d.Hc, 1, a.seed, 1, step, k, thr_gcn, 1.f / (1.f - a.p_gcn),
                               base));
    from = to;
  }
}

// The statistics kernel of more than 32 members needs its dynamic-LDS limit raised, once per context.
int raise_stats_lds(bool* set, int E, hipError_t (*prepare)(), const char* entry, const char* kernel) {
  if (E <= 32 || *set) return SMAML_OK;
  const hipError_t st = prepare();
  if (st != hipSuccess)
    return fail(SMAML_EHIP, std::string(entry) + ": raising " + kernel + "'s dynamic LDS limit to 64 KB (more than 32 "
                                "members) failed: " + hipGetErrorString(st));
  *set = true;
  return SMAML_OK;
}

// The per-layer GCN chain over `ns` samples of rps rows each that start at tab[i] (the first ell_rows of each
// aggregate over the graph), time-major into dst over all ns samples; in chunks of samples whose buffers stay
// below 2^30 bytes (the layer kernel's loaders index in 32 bits). drop_rps: launch_gcn_layer's.
void gcn_chain(smaml_ctx* c, hipStream_t s, const float* const* tab, int ns, int rps, int ell_rows, int drop_rps,
               float* dst) {
  const Dims& d = c->d;
  const GraphView gv = graph_view(c);
  float* bufs[2] = {c->w.gcnA, c->w.gcnB};
  const int cs = (int)std::max<int64_t>(1, (1ll << 28) / ((int64_t)rps * d.Hc));
  for (int s0 = 0; s0 < ns; s0 += cs) {
    const int n = std::min(cs, ns - s0);
    const float* from = nullptr;
    for (int k = 0; k < 4; ++k) {
      const bool last = k == 3;
      float* to = last ? dst + (int64_t)s0 * d.N * d.Hc : bufs[k & 1];
      TIMED(c, s, C_GCN, 2.0 * n * rps * c->go.cin[k] * d.Hc,
            launch_gcn_layer(s, d, k, n, ns, k == 0 ? tab + s0 : nullptr, from, to, last, true, c->gcn + c->go.w[k],
                             c->gcn + c->go.b[k], c->go.cin[k], d.Hc, gv, rps, ell_rows, nullptr, drop_rps));
      from = to;
    }
  }
}

// -- stages of the two rollouts --
// First private row whose features cycle j computes: with reuse only the rows the previous cycle appended
// that the window's steps t >= 1 read (all of them when T > s; when T <= s the window holds fewer rows than a
// cycle appends), else every row t >= 1 of the window. The run ends at row j s + T - 1.
int roll_run_first(int j, int T, int sl, bool reuse) {
  if (j == 0 || !reuse) return j * sl + 1;
  return std::max(j * sl + 1, (j - 1) * sl + T);
}

// What a rollout call fixes for all its passes. G members of a group run side by side (1: the deterministic
// rollout). The uploaded table: src[norig] (origin rows); ensemble: obs[norig] (the same one step on); then one
// set per pass size -- tabB[0] = Bmax and, where the ensemble's last pass is smaller, tabB[1] behind it -- of per
// cycle win[G * B], run[G * B], entry z * B + b. The deterministic rollout reads its tail pass from the one set.
struct RollPlan {
  int Bmax = 0, Btail = 0, S = 0, G = 1;
  bool reuse = true, fused = false;
  int64_t tab_src = 0, tab_obs = 0, tab_cyc[2] = {0, 0};
  int tabB[2] = {0, 0};
};

RollPlan roll_plan(const smaml_ctx* c, const ForecastCall& a) {
  RollPlan p{};
  p.Bmax = std::min(a.batch, a.n);
  p.Btail = a.ens && a.n % a.batch ? a.n % a.batch : p.Bmax;
  p.S = c->d.T;
  p.reuse = c->roll_reuse != 0;
  p.fused = gcn_mlp_supported(c->d) && c->kn.gcn_fused;
  return p;
}

// Builds the table described at RollPlan over the private sequences seq [G * Bmax][seq_rows][N][Cin0] and
// records where its parts start.
std::vector<const float*> roll_table(const smaml_ctx* c, const ForecastCall& a, const float* seq, RollPlan& p) {
  const Dims& d = c->d;
  const int sl = d.Hf + 1, R = a.cycles, nset = p.Btail != p.Bmax ? 2 : 1;
  const int64_t rowf = (int64_t)d.N * d.Cin0, seq_rows = roll_seq_rows(d, R), head = (a.ens ? 2 : 1) * (int64_t)a.n;
  std::vector<const float*> ptrs((size_t)head + (size_t)R * 2 * p.G * (p.Bmax + (nset == 2 ? p.Btail : 0)));
  for (int i = 0; i < a.n; ++i) {
    ptrs[i] = c->feats[a.task] + (int64_t)a.list[i] * rowf;
    if (a.ens) ptrs[(size_t)a.n + i] = ptrs[i] + rowf;
  }
  p.tab_src = 0;
  p.tab_obs = a.n;
  // without a set of its own a smaller last pass reads set 0, at set 0's stride (entry z * Bmax + b, b < B)
  p.tab_cyc[0] = p.tab_cyc[1] = head;
  p.tabB[0] = p.tabB[1] = p.Bmax;
  int64_t at = head;
  for (int k = 0; k < nset; ++k) {
    if (k == 1) {
      p.tab_cyc[1] = at;
      p.tabB[1] = p.Btail;
    }
    const int GB = p.G * p.tabB[k];
    for (int j = 0; j < R; ++j)
      for (int zb = 0; zb < GB; ++zb) {
        const float* sb = seq + (int64_t)zb * seq_rows * rowf;
        ptrs[(size_t)(at + ((int64_t)j * 2) * GB + zb)] = sb + (int64_t)j * sl * rowf;
        ptrs[(size_t)(at + ((int64_t)j * 2 + 1) * GB + zb)] = sb + (int64_t)roll_run_first(j, d.T, sl, p.reuse) * rowf;
      }
    at += (int64_t)R * 2 * GB;
  }
  return ptrs;
}

// cycle j's window (win) and run tables of a pass of B origins
int roll_tabs(const smaml_ctx* c, const RollPlan& p, int j, int B, const float* const** win, const float* const** run) {
  const int k = B == p.Bmax ? 0 : 1;
  const int64_t GB = (int64_t)p.G * p.tabB[k];
  TRY(xtab_at(c, p.tab_cyc[k] + (int64_t)j * 2 * GB, win));
  TRY(xtab_at(c, p.tab_cyc[k] + ((int64_t)j * 2 + 1) * GB, run));
  return SMAML_OK;
}

// What a rollout pass's stages share: the GCN weight offsets, layer 0's gate image and the sequence addressing
struct RollSetup {
  GcnWOff wo;
  const char* gimg = nullptr;
  int64_t gimg_off = 0;
  RollArgs ra;
};

// c->w and the gate images for a pass of B origins with rows from src, the fused stack's weight image (wsplit),
// and the addressing of the private sequences seq.
int roll_setup(smaml_ctx* c, hipStream_t s, const float* theta, int B, int R, float* seq, const float* const* src,
               bool wsplit, RollSetup* rs) {
  const Dims& d = c->d;
  forecast_work(c, B);
  TRY(prep_gate_images(c, s, theta, 0));
  const Work& cw = c->w;
  rs->gimg = cw.gimg.th && cw.gimg_src == theta ? cw.gimg.th : nullptr;
  rs->gimg_off = cw.gimg.off[0][0];
  for (int k = 0; k < 4; ++k) {
    rs->wo.w[k] = c->go.w[k];
    rs->wo.b[k] = c->go.b[k];
  }
  if (wsplit) TIMED(c, s, C_MISC, 0, launch_gcn_wsplit(s, d, c->gcn, rs->wo, c->gcn_wimg.as<char>()));
  RollArgs& ra = rs->ra;
  ra = RollArgs{};
  ra.seq = seq;
  ra.seq_rows = (int)roll_seq_rows(d, R);
  ra.seq_stride = (int64_t)ra.seq_rows * d.N * d.Cin0;
  ra.src = src;
  ra.B = B;
  ra.N = d.N;
  ra.Cin = d.Cin0;
  ra.C = d.C;
  ra.Hf = d.Hf;
  ra.T = d.T;
  return SMAML_OK;
}

// The four position-independent convs of `nrun` rows t >= 1 of each of ns samples (from tab[i]), time-major
// into F: the fused stack, or the per-layer chain
void gcn_rows(smaml_ctx* c, hipStream_t s, const RollSetup& rs, bool fused, const float* const* tab, int ns, int nrun,
              int drop_rps, float* F) {
  const Dims& d = c->d;
  if (fused)
    TIMED(c, s, C_GCN, 2.0 * ns * nrun * d.N * d.Hc * (d.Cin0 + 3.0 * d.Hc),
          launch_gcn_mlp_run(s, d, ns, nrun, tab, c->gcn, rs.wo, c->gcn_wimg.as<char>(), F));
  else
    gcn_chain(c, s, tab, ns, nrun * d.N, 0, drop_rps, F);
}

// Layer 0's projection of plain rows F [rows][Hc] into out [rows][4H], in launches whose output stays below
// 2^32 bytes (k_xg_dedup's stores index in 32 bits). blocks (optional) += the N-row blocks projected.
void xg_rows(smaml_ctx* c, hipStream_t s, const float* theta, const RollSetup& rs, const float* F, int64_t rows,
             float* out, int64_t* blocks) {
  const Dims& d = c->d;
  const int64_t cr = ((1ll << 30) / (4 * d.H) - 1) / 256 * 256;
  for (int64_t r = 0; r < rows; r += cr) {
    const int64_t n = std::min(cr, rows - r);
    TIMED(c, s, C_XG, 2.0 * n * 4 * d.H * c->po.lay[0].cin,
          launch_xg_rows(s, d, c->w, F + r * d.Hc, n, theta, c->po, rs.gimg, rs.gimg_off, out + r * 4 * d.H));
  }
  if (blocks) *blocks += rows / d.N;
}

// The projection of a run of nrun steps (F time-major, gM rows per step) into the slots of the ring table xg
// [S][gM][4H] from row r0 on: a run that wraps the table takes two launches
void xg_run_slots(smaml_ctx* c, hipStream_t s, const float* theta, const RollSetup& rs, const float* F, int r0,
                  int nrun, int S, int64_t gM, float* xg, int64_t* blocks) {
  const Dims& d = c->d;
  for (int tau = 0; tau < nrun;) {
    const int sl0 = (r0 + tau) % S, len = std::min(nrun - tau, S - sl0);
    xg_rows(c, s, theta, rs, F + (int64_t)tau * gM * d.Hc, (int64_t)len * gM, xg + (int64_t)sl0 * gM * 4 * d.H, blocks);
    tau += len;
  }
}

// -- the pass functions --
// One pass of B windows of one stream (xt: their device pointer table; consec: w[b] = w[0] + b): GCN, layer
// 0's projection per distinct stream row (consecutive passes), the inference wavefront, the head into
// pred_out [B][N*Hf][C] and, with skill, the pass's sums added onto it.
int forecast_pass(smaml_ctx* c, hipStream_t s, const float* theta, const float* const* xt, int B, bool consec,
                  float* pred_out, const float* scale_dev, double* skill, bool first) {
  const Dims& d = c->d;
  const int M = B * d.N;
  const FeatPlan f = feat_plan(c, B, consec);
  const int64_t ring = infer_ring_floats(d, 1, M);
  if (c->fc_ring.grow(2 * ring * 4) != hipSuccess || c->fc_F.grow(f.frows * d.Hc * 4) != hipSuccess ||
      grow_all<HipAlloc>({{&c->fc_gcnA, f.grows * d.Hc * 4}, {&c->fc_gcnB, f.grows * d.Hc * 4}}) != hipSuccess ||
      (!pred_out && c->fc_pred.grow((int64_t)M * d.HfC * 4) != hipSuccess) ||
      (skill && c->fc_part.grow((int64_t)skill_blocks(d, B) * d.HfC * 3 * 4) != hipSuccess))
    return fail(SMAML_ENOMEM, "hipMalloc of the forecast buffers failed (batch " + std::to_string(B) + ")");
  forecast_work(c, B);
  TRY(shared_features(c, s, theta, xt, consec, f));
  float* ringH = c->fc_ring.as<float>();
  float* pred = pred_out ? pred_out : c->fc_pred.as<float>();
  infer_waves(c, s, theta, ringH, ringH + ring, pred);
  if (skill)
    TIMED(c, s, C_MISC, 0,
          launch_skill_sums(s, d, B, pred, xt, scale_dev, c->fc_part.as<float>(), skill, first, score_weights(c)));
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

// Members of one launch set for a pass of M rows: `want` (option ens_group; 0 = all), else the largest
// group whose rings -- and, with GCN dropout, per-member features -- stay within ENS_GROUP_BUDGET.
constexpr int64_t ENS_GROUP_BUDGET = 2ll << 30;
int ens_group_size(const Dims& d, int M, int E, bool per_member_F, int want) {
  if (want > 0) return std::min(want, E);
  if (want == 0) return E;
  const int64_t per = 2 * infer_ring_floats(d, 1, M) * 4 + (per_member_F ? (int64_t)d.T * M * d.Hc * 4 : 0);
  return (int)std::max<int64_t>(1, std::min<int64_t>(E, ENS_GROUP_BUDGET / per));
}

// One pass of B windows (first of them `done` in the call's list) for all E members. p_gcn == 0: the shared
// features of forecast_pass once for all members, layer 0 of the LSTM once (option ens_share), layers >= 1 with
// grid z = member. p_gcn > 0: each member's masked GCN into its own F. The members' predictions go to
// c->ens_pred [E][B][N*Hf][C], from which k_ens_stats forms every output.
int ensemble_pass(smaml_ctx* c, hipStream_t s, const float* theta, const float* const* xt, int B, bool consec,
                  const ForecastCall& a, int64_t done, const float* scale_dev, float* mean, float* spread,
                  float* member_pred, double* scores) {
  const Dims& d = c->d;
  const int M = B * d.N, E = a.members;
  const bool shared = a.p_gcn == 0.f;
  const int G = ens_group_size(d, M, E, !shared, c->ens_group);
  const int64_t fslab = (int64_t)d.T * M * d.Hc;  // floats of one member's own features
  FeatPlan f;
  if (shared) f = feat_plan(c, B, consec);
  else f.frows = f.grows = (int64_t)d.T * M;
  const int64_t ring = infer_ring_floats(d, G, M);
  if (c->ens_ring.grow(2 * ring * 4) != hipSuccess ||
      c->fc_F.grow((shared ? f.frows * d.Hc : G * fslab) * 4) != hipSuccess ||
      grow_all<HipAlloc>({{&c->fc_gcnA, f.grows * d.Hc * 4}, {&c->fc_gcnB, f.grows * d.Hc * 4}}) != hipSuccess ||
      c->ens_pred.grow((int64_t)E * M * d.HfC * 4) != hipSuccess ||
      (scores && c->fc_part.grow((int64_t)skill_blocks(d, B) * d.HfC * 4 * 4) != hipSuccess))
    return fail(SMAML_ENOMEM, "hipMalloc of the ensemble buffers failed (batch " + std::to_string(B) + ", " +
                                  std::to_string(G) + " members at a time)");
  forecast_work(c, B);
  if (shared) TRY(shared_features(c, s, theta, xt, consec, f));
  else TRY(prep_gate_images(c, s, theta, 0));
  EnsDrop ed = ens_drop(d, a, done);
  // (a one-layer LSTM has no layer above to read a shared layer 0: its layer 0 is the top layer, whose h_T
  // every member masks and hands to the head itself)
  ed.share0 = shared && c->ens_share && d.L > 1 ? 1 : 0;
  float* ringH = c->ens_ring.as<float>();
  float* P = c->ens_pred.as<float>();
  for (int e0 = 0; e0 < E; e0 += G) {
    const int g = std::min(G, E - e0);
    if (!shared)  // member e0 + z's masks are those of step e0 + z
      for (int z = 0; z < g; ++z)
        member_gcn_masked(c, s, xt, a, e0 + z, (uint64_t)done * d.T * d.N * d.Hc, c->w.F + (int64_t)z * fslab);
    ed.e0 = e0;
    // (the rings are laid out for g members, the cell states behind a full group's)
    infer_waves_drop(c, s, theta, ringH, ringH + ring, g, shared ? 0 : fslab, ed, P + (int64_t)e0 * M * d.HfC);
  }
  TRY(raise_stats_lds(&c->ens_lds_set, E, ens_stats_prepare, "smaml_forecast_ensemble", "k_ens_stats"));
  TIMED(c, s, C_MISC, 0,
        launch_ens_stats(s, d, B, E, P, xt, scale_dev, mean, spread, member_pred, (int64_t)a.n * d.N * d.HfC,
                         c->fc_part.as<float>(), scores, done == 0, scores ? score_weights(c) : nullptr));
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

// One pass of B origins (first of them `done` in the call's list) through the R cycles in lockstep: per cycle
// the features and projections the window owes, the wavefront and head, and the forecast appended to every
// origin's sequence.
int rollout_pass(smaml_ctx* c, hipStream_t s, const ForecastCall& a, const RollPlan& p, int64_t done, int B,
                 const float* scale_dev, float* traj, double* skill) {
  const Dims& d = c->d;
  const float* theta = a.theta;
  const int M = B * d.N, sl = d.Hf + 1, S = p.S, R = a.cycles;
  const int64_t ring = infer_ring_floats(d, 1, M), blkf = (int64_t)sl * d.N * d.C, slot = (int64_t)M * 4 * d.H;
  const float* const* src = nullptr;
  TRY(xtab_at(c, p.tab_src + done, &src));
  RollSetup rs;
  TRY(roll_setup(c, s, theta, B, R, c->ro_seq.as<float>(), src, p.fused, &rs));
  Work& cw = c->w;
  TIMED(c, s, C_MISC, 0, launch_rollout_init(s, rs.ra));
  float* xg = c->ro_xg.as<float>();
  float* xg0 = xg + (int64_t)S * slot;
  float* F0 = c->ro_F0.as<float>();
  float* ringH = c->fc_ring.as<float>();
  float* pred = c->fc_pred.as<float>();
  for (int j = 0; j < R; ++j) {
    const float* const* wtab = nullptr;
    const float* const* rtab = nullptr;
    TRY(roll_tabs(c, p, j, B, &wtab, &rtab));
    // the rows t >= 1 this cycle owes: the four position-independent convs, then layer 0's projection into
    // their slots
    const int r0 = roll_run_first(j, d.T, sl, p.reuse), nrun = j * sl + d.T - r0;
    if (nrun > 0) {
      gcn_rows(c, s, rs, p.fused, rtab, B, nrun, 0, cw.F);
      xg_run_slots(c, s, theta, rs, cw.F, r0, nrun, S, M, xg, nullptr);
      c->ro_stats[1] += (int64_t)B * nrun;
      c->ro_stats[3] += (int64_t)B * nrun;
    }
    // the t = 0 rows aggregate over the graph (F3): per-layer chain over N-row blocks, as run_gcn's
    gcn_chain(c, s, wtab, B, d.N, d.N, d.T * d.N, F0);
    xg_rows(c, s, theta, rs, F0, M, xg0, nullptr);
    c->ro_stats[2] += B;
    c->ro_stats[3] += B;
    XgDedup xd{};
    xd.xg = xg;
    xd.xg0 = xg0;
    xd.src = theta;
    xd.N = d.N;
    xd.ring_S = S;
    xd.ring_r0 = (j * sl) % S;
    cw.xgd = xd;
    infer_waves(c, s, theta, ringH, ringH + ring, pred);
    float* out = traj ? traj + ((int64_t)done * R + j) * blkf : c->ro_blk.as<float>();
    const int64_t ostride = traj ? (int64_t)R * blkf : blkf;
    TIMED(c, s, C_MISC, 0, launch_rollout_append(s, rs.ra, j, a.gap, j + 1 < R, pred, out, ostride));
    c->ro_stats[4] += 1;
    if (skill)
      TIMED(c, s, C_MISC, 0,
            launch_rollout_skill(s, rs.ra, j, R, out, ostride, scale_dev, c->fc_part.as<float>(), skill, done == 0,
                                 score_weights(c)));
    c->ro_stats[0] += 1;
  }
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

// floats of one member of a pass of M rows: rings, slot table with its t = 0 block, sequences, features
int64_t rens_member_bytes(const Dims& d, int B, int R, bool per_member_F) {
  const int64_t M = (int64_t)B * d.N, sl = d.Hf + 1;
  const int64_t f = 2 * infer_ring_floats(d, 1, (int)M) + (d.T + 1) * M * 4 * d.H +
                    (int64_t)B * (d.T + (int64_t)(R - 1) * sl) * d.N * d.Cin0 +
                    (per_member_F ? (int64_t)d.T : std::max(d.T - 1, 1)) * M * d.Hc + M * d.Hc;
  return f * 4;
}

// One pass of B origins (first of them `done`): the members G at a time over grid z, every (member, origin)
// pair of a group in lockstep through the R cycles; then the pass's statistics from all E trajectories.
// p_gcn == 0: rollout_pass's stages over g B samples, less what every member reads unchanged (with reuse: the
// observed rows and cycle 0's t = 0 block, once for the pass). p_gcn > 0: ensemble_pass's masked GCN per
// member and cycle.
int rens_pass(smaml_ctx* c, hipStream_t s, const ForecastCall& a, const RollPlan& p, int64_t done, int B,
              const float* scale_dev, float* member_traj, float* mean, float* spread, double* scores) {
  const Dims& d = c->d;
  const float* theta = a.theta;
  const int M = B * d.N, sl = d.Hf + 1, S = p.S, E = a.members, R = a.cycles, TN = d.T * d.N;
  const bool shared = a.p_gcn == 0.f, obs = shared && p.reuse;
  const int64_t blkf = (int64_t)sl * d.N * d.C, slot = (int64_t)M * 4 * d.H, fslab = (int64_t)d.T * M * d.Hc;
  const float* const* src = nullptr;
  const float* const* otab = nullptr;
  TRY(xtab_at(c, p.tab_src + done, &src));
  TRY(xtab_at(c, p.tab_obs + done, &otab));
  RollSetup rs;
  TRY(roll_setup(c, s, theta, B, R, c->re_seq.as<float>(), src, shared && p.fused, &rs));
  Work& cw = c->w;
  float* Frun = cw.F;
  float* xobs = c->re_obs.as<float>();
  float* xobs0 = xobs + (int64_t)d.T * slot;
  float* F0 = c->re_F0.as<float>();
  int64_t* xg_blocks = &c->re_stats[4];
  if (obs) {
    // what every member reads unchanged: the observed rows 1 .. T - 1 (position-independent GCN, projection)
    // and cycle 0's t = 0 block, once for the pass
    const int nobs = d.T - 1;
    if (nobs > 0) {
      gcn_rows(c, s, rs, p.fused, otab, B, nobs, TN, Frun);
      xg_rows(c, s, theta, rs, Frun, (int64_t)nobs * M, xobs + slot, xg_blocks);
      c->re_stats[2] += (int64_t)B * nobs;
    }
    gcn_chain(c, s, src, B, d.N, d.N, TN, F0);
    xg_rows(c, s, theta, rs, F0, M, xobs0, xg_blocks);
    c->re_stats[3] += B;
  }
  float* traj = member_traj ? member_traj + done * R * blkf : c->re_traj.as<float>();
  const int64_t tstride = (member_traj ? (int64_t)a.n : (int64_t)B) * R * blkf;  // floats between two members
  EnsDrop ed = ens_drop(d, a, done);
  float* P = c->ens_pred.as<float>();
  for (int e0 = 0; e0 < E; e0 += p.G) {
    const int g = std::min(p.G, E - e0);
    float* ringH = c->ens_ring.as<float>();
    float* ringC = ringH + infer_ring_floats(d, g, M);
    float* xg = c->re_xg.as<float>();           // [S][g][M][4H]
    float* xg0 = xg + (int64_t)S * g * slot;    // [g][M][4H]
    TIMED(c, s, C_MISC, 0, launch_rollout_init(s, rs.ra, g));
    c->re_stats[6] += 1;
    for (int j = 0; j < R; ++j) {
      const float* const* wtab = nullptr;
      const float* const* rtab = nullptr;
      TRY(roll_tabs(c, p, j, B, &wtab, &rtab));
      const bool first_shared = obs && j == 0;  // every block of cycle 0 is in the shared table
      if (!shared) {
        // each member's GCN under its own kind-1 masks of step 64 j + e: all T rows of its window, every cycle
        for (int z = 0; z < g; ++z)
          member_gcn_masked(c, s, wtab + (int64_t)z * B, a, 64 * j + e0 + z, (uint64_t)done * TN * d.Hc,
                            Frun + (int64_t)z * fslab);
        c->re_stats[1] += (int64_t)g * B * (d.T - 1);
        c->re_stats[3] += (int64_t)g * B;
        cw.xgd = XgDedup{};
      } else {
        if (!first_shared) {
          // the rows t >= 1 the members owe (with reuse: those they appended in the previous cycle), g B samples
          // in one launch, time-major over the group, then into their slots; then their t = 0 blocks
          const int r0 = roll_run_first(j, d.T, sl, p.reuse), nrun = j * sl + d.T - r0;
          if (nrun > 0) {
            gcn_rows(c, s, rs, p.fused, rtab, g * B, nrun, TN, Frun);
            xg_run_slots(c, s, theta, rs, Frun, r0, nrun, S, (int64_t)g * M, xg, xg_blocks);
            c->re_stats[1] += (int64_t)g * B * nrun;
          }
          gcn_chain(c, s, wtab, g * B, d.N, d.N, TN, F0);
          xg_rows(c, s, theta, rs, F0, (int64_t)g * M, xg0, xg_blocks);
          c->re_stats[3] += (int64_t)g * B;
        }
        XgDedup xd{};
        xd.xg = xg;
        xd.xg0 = first_shared ? xobs0 : xg0;
        xd.src = theta;
        xd.N = d.N;
        xd.ring_S = S;
        cw.xgd = xd;
        ed.xg0_z = first_shared ? 0 : slot;
        ed.xg_obs = obs ? xobs : nullptr;
        ed.obs_rows = obs ? d.T : 0;
        ed.ring_row = j * sl;
      }
      ed.e0 = 64 * j + e0;
      // cycle 0's windows are the same in every member: with nothing masked below layer 0's output, layer 0 once
      ed.share0 = shared && j == 0 && c->ens_share && d.L > 1 ? 1 : 0;
      infer_waves_drop(c, s, theta, ringH, ringC, g, shared ? 0 : fslab, ed, P);
      TIMED(c, s, C_MISC, 0,
            launch_rollout_append(s, rs.ra, j, a.gap, j + 1 < R, P, traj + e0 * tstride + (int64_t)j * blkf,
                                  (int64_t)R * blkf, g, tstride));
      c->re_stats[5] += 1;
      c->re_stats[0] += 1;
    }
  }
  if (mean || spread || scores) {
    TRY(raise_stats_lds(&c->rens_lds_set, E, rens_stats_prepare, "smaml_forecast_rollout_ensemble", "k_rens_stats"));
    const int64_t off = done * R * blkf;
    TIMED(c, s, C_MISC, 0,
          launch_rens_stats(s, d, B, E, R * sl, traj, tstride, src, scale_dev, mean ? mean + off : nullptr,
                            spread ? spread + off : nullptr, c->fc_part.as<float>(), scores, done == 0,
                            scores ? score_weights(c) : nullptr));
  }
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

}  // namespace

// =====================================================================================
extern "C" {

const char* smaml_last_error(void) { return g_err.c_str(); }

int32_t smaml_abi_version(void) { return 9; }

const char* smaml_build_info(void) { return smaml::products_info(); }

int smaml_param_layout(const smaml_dims* dims, int32_t which, int64_t* offsets, int64_t* sizes, int32_t cap,
                       int32_t* count, int64_t* total) {
  TRY(check_dims(dims));
  if (which != 0 && which != 1) return fail(SMAML_EINVAL, "which must be 0 (trainable) or 1 (gcn)");
  std::vector<Spec> sp;
  int64_t tot = 0;
  layout(*dims, which, sp, tot);
  if (count) *count = (int32_t)sp.size();
  if (total) *total = tot;
  for (int i = 0; i < (int)sp.size() && i < cap; ++i) {
    if (offsets) offsets[i] = sp[i].off;
    if (sizes) sizes[i] = sp[i].size;
  }
  return SMAML_OK;
}

int smaml_graph_ell(const int64_t* edge_index_host, int64_t num_edges, int32_t num_nodes, int32_t* cols_host,
                    float* vals_host) {
  if (!edge_index_host || !cols_host || !vals_host || num_nodes <= 0 || num_edges < 0)
    return fail(SMAML_EINVAL, "bad arguments to smaml_graph_ell");
  std::vector<int32_t> cols;
  std::vector<float> vals;
  TRY(build_ell(edge_index_host, num_edges, num_nodes, cols, vals));
  std::memcpy(cols_host, cols.data(), cols.size() * 4);
  std::memcpy(vals_host, vals.data(), vals.size() * 4);
  return SMAML_OK;
}

int smaml_create(const smaml_dims* dims, int32_t device, smaml_ctx** out) {
  if (!out) return fail(SMAML_EINVAL, "out is NULL");
  *out = nullptr;
  TRY(check_dims(dims));
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(SMAML_EINVAL, "device ordinal out of range");
  smaml_ctx* c = new smaml_ctx();
  c->dims = *dims;
  c->device = device;
  Dims& d = c->d;
  d.N = dims->num_nodes;
  d.T = dims->window_size;
  d.Cin0 = dims->input_channels;
  d.Hc = dims->hidden_channels;
  d.H = dims->lstm_hidden_size;
  d.L = dims->lstm_num_layers;
  d.Hf = dims->forecast_horizon;
  d.C = dims->output_channels;
  d.HfC = d.Hf * d.C;
  std::vector<Spec> sp;
  int64_t tot = 0;
  layout(*dims, 0, sp, tot);
  for (int l = 0; l < d.L; ++l) {
    c->po.lay[l].wih = sp[4 * l].off;
    c->po.lay[l].whh = sp[4 * l + 1].off;
    c->po.lay[l].bih = sp[4 * l + 2].off;
    c->po.lay[l].bhh = sp[4 * l + 3].off;
    c->po.lay[l].cin = l == 0 ? d.Hc : d.H;
  }
  c->po.wo = sp[4 * d.L].off;
  c->po.bo = sp[4 * d.L + 1].off;
  c->po.P = tot;
  int64_t nv = 0;
  for (auto& x : sp) nv += x.size;
  c->po.n_valid = nv;
  layout(*dims, 1, sp, tot);
  for (int k = 0; k < 4; ++k) {
    c->go.b[k] = sp[2 * k].off;
    c->go.w[k] = sp[2 * k + 1].off;
    c->go.cin[k] = k == 0 ? d.Cin0 : d.Hc;
  }
  c->go.total = tot;
  if (const char* e = std::getenv("SMAML_BWD_BIG_MIN")) c->kn.bwd_big_min = std::atoi(e);
  if (const char* e = std::getenv("SMAML_BWDD_BIG_MIN")) c->kn.bwdd_big_min = std::atoi(e);
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    delete c;
    return fail(SMAML_EHIP, std::string("context init: ") + hipGetErrorString(e));
  }
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) c->n_cu = ncu;
  *out = c;
  return SMAML_OK;
}

int smaml_destroy(smaml_ctx* c) {
  if (!c) return SMAML_OK;
  (void)hipSetDevice(c->device);
  if (c->comm) (void)smaml_comm_destroy(c);
  (void)hipDeviceSynchronize();
  (void)c->stage.release();
  for (int i = 0; i < 4; ++i) {
    if (c->cs[i]) (void)hipStreamDestroy(c->cs[i]);
    if (c->join_ev[i]) (void)hipEventDestroy(c->join_ev[i]);
  }
  if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
  if (c->gc_ev) (void)hipEventDestroy(c->gc_ev);
  if (c->bar_err_host) (void)hipHostFree(c->bar_err_host);
  for (auto& r : c->tm.recs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  for (auto e : c->tm.pool) (void)hipEventDestroy(e);
  delete c;  // (every HipBuf releases its memory)
  return SMAML_OK;
}

// Upload A_hat^T (both forms' backward aggregation) and record the graph's counters; the caller has uploaded
// A_hat's own table. Everything that can fail on the host has happened before the first of these calls.
static int upload_transpose(smaml_ctx* c, int form, const std::vector<int32_t>& rowptr, const std::vector<int32_t>& tp,
                            const std::vector<int32_t>& tc, const std::vector<float>& tv) {
  HIP_TRY(hipMemcpy(c->tr_p.ptr, tp.data(), tp.size() * 4, hipMemcpyHostToDevice));
  if (!tc.empty()) {
    HIP_TRY(hipMemcpy(c->tr_c.ptr, tc.data(), tc.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->tr_v.ptr, tv.data(), tv.size() * 4, hipMemcpyHostToDevice));
  }
  int32_t longest = 0;
  for (size_t t = 0; t + 1 < rowptr.size(); ++t) longest = std::max(longest, rowptr[t + 1] - rowptr[t]);
  c->graph_form = form;
  c->graph_stats[0] = form;
  c->graph_stats[1] = rowptr.back();
  c->graph_stats[2] = longest;
  c->graph_stats[3] = c->graph_stats[4] = 0;
  return SMAML_OK;
}

int smaml_set_graph(smaml_ctx* c, const int64_t* edge_index_host, int64_t num_edges) {
  if (!c || !edge_index_host) return fail(SMAML_EINVAL, "NULL argument");
  TRY(ensure_device(c));
  std::vector<int32_t> cols;
  std::vector<float> vals;
  TRY(build_ell(edge_index_host, num_edges, c->d.N, cols, vals));
  ad_cache_invalidate(c);
  gc_invalidate(c);
  const int N = c->d.N;
  std::vector<int32_t> rp, rc, tp, tc;
  std::vector<float> rv, tv;
  ell_to_csr(N, cols, vals, rp, rc, rv);
  csr_transpose(N, rp, rc, rv, tp, tc, tv);
  const int64_t ell = (int64_t)cols.size() * 4, nnz = std::max<int64_t>((int64_t)tc.size(), 1) * 4;
  HIP_TRY(grow_all<HipAlloc>(
      {{&c->ell_c, ell}, {&c->ell_v, ell}, {&c->tr_p, (int64_t)tp.size() * 4}, {&c->tr_c, nnz}, {&c->tr_v, nnz}}));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(c->ell_c.ptr, cols.data(), cols.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->ell_v.ptr, vals.data(), vals.size() * 4, hipMemcpyHostToDevice));
  return upload_transpose(c, 1, rp, tp, tc, tv);
}

int smaml_graph_csr(const int64_t* edge_index_host, const float* edge_weight_host, int64_t num_edges, int32_t num_nodes,
                    int32_t* rowptr_host, int32_t* cols_host, float* vals_host, int64_t cap, int64_t* nnz_out) {
  if (nnz_out) *nnz_out = 0;
  if (!edge_index_host || !rowptr_host || !nnz_out || num_nodes <= 0 || num_edges < 0 || cap < 0 ||
      (cap > 0 && (!cols_host || !vals_host)))
    return fail(SMAML_EINVAL, "bad arguments to smaml_graph_csr");
  std::vector<int32_t> rp, cols;
  std::vector<float> vals;
  TRY(build_csr(edge_index_host, edge_weight_host, num_edges, num_nodes, rp, cols, vals));
  *nnz_out = (int64_t)cols.size();
  if ((int64_t)cols.size() > cap)
    return fail(SMAML_EINVAL, "smaml_graph_csr: cap (" + std::to_string(cap) + ") is below the graph's " +
                                  std::to_string(cols.size()) + " entries");
  std::memcpy(rowptr_host, rp.data(), rp.size() * 4);
  if (!cols.empty()) {
    std::memcpy(cols_host, cols.data(), cols.size() * 4);
    std::memcpy(vals_host, vals.data(), vals.size() * 4);
  }
  return SMAML_OK;
}

int smaml_set_graph_weighted(smaml_ctx* c, const int64_t* edge_index_host, const float* edge_weight_host,
                             int64_t num_edges) {
  if (!c || !edge_index_host || num_edges < 0) return fail(SMAML_EINVAL, "bad arguments to smaml_set_graph_weighted");
  TRY(ensure_device(c));
  const int N = c->d.N;
  std::vector<int32_t> rp, rc, tp, tc;
  std::vector<float> rv, tv;
  TRY(build_csr(edge_index_host, edge_weight_host, num_edges, N, rp, rc, rv));
  ad_cache_invalidate(c);
  gc_invalidate(c);
  csr_transpose(N, rp, rc, rv, tp, tc, tv);
  const int64_t nnz = std::max<int64_t>((int64_t)rc.size(), 1) * 4, np = (int64_t)rp.size() * 4;
  HIP_TRY(grow_all<HipAlloc>(
      {{&c->csr_p, np}, {&c->csr_c, nnz}, {&c->csr_v, nnz}, {&c->tr_p, np}, {&c->tr_c, nnz}, {&c->tr_v, nnz}}));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(c->csr_p.ptr, rp.data(), rp.size() * 4, hipMemcpyHostToDevice));
  if (!rc.empty()) {
    HIP_TRY(hipMemcpy(c->csr_c.ptr, rc.data(), rc.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->csr_v.ptr, rv.data(), rv.size() * 4, hipMemcpyHostToDevice));
  }
  return upload_transpose(c, 2, rp, tp, tc, tv);
}

int smaml_graph_stats(const smaml_ctx* c, int64_t* counts, int32_t cap, int32_t* count) {
  if (!c || cap < 0 || (cap > 0 && !counts)) return fail(SMAML_EINVAL, "bad graph_stats arguments");
  for (int i = 0; i < 5 && i < cap; ++i) counts[i] = c->graph_stats[i];
  if (count) *count = 5;
  return SMAML_OK;
}

// One weight vector: every entry finite and >= 0, at least one positive. `what` names it in the message.
static int check_weights(const float* w, int64_t n, const std::string& what) {
  bool positive = false;
  for (int64_t i = 0; i < n; ++i) {
    if (!(w[i] >= 0.f) || std::isinf(w[i]))
      return fail(SMAML_EINVAL, what + " element " + std::to_string(i) + " is " + std::to_string(w[i]) +
                                    " (weights are finite and >= 0)");
    positive = positive || w[i] > 0.f;
  }
  if (!positive) return fail(SMAML_EINVAL, what + " has no positive weight");
  return SMAML_OK;
}

int smaml_loss_weights_check(const smaml_dims* dims, const float* w_host, int32_t nsets) {
  if (!dims || !w_host) return fail(SMAML_EINVAL, "smaml_loss_weights_check: NULL argument");
  if (nsets <= 0) return fail(SMAML_EINVAL, "smaml_loss_weights_check: nsets must be positive");
  const int64_t per = (int64_t)dims->forecast_horizon * dims->num_nodes * dims->output_channels;
  if (per <= 0) return fail(SMAML_EINVAL, "smaml_loss_weights_check: bad dims");
  for (int32_t z = 0; z < nsets; ++z)
    TRY(check_weights(w_host + (int64_t)z * per, per, "loss weights: set " + std::to_string(z)));
  return SMAML_OK;
}

int smaml_set_loss_weights(smaml_ctx* c, const float* w_host, int32_t nsets) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  if (w_host || nsets != 0) {
    TRY(smaml_loss_weights_check(&c->dims, w_host, nsets));  // (a failure leaves the live table alone)
    TRY(ensure_device(c));
    const int64_t bytes = (int64_t)nsets * c->d.Hf * c->d.N * c->d.C * 4;
    HIP_TRY(hipDeviceSynchronize());  // (nothing that reads the old table is in flight)
    HIP_TRY(c->lw_buf.grow(bytes));
    HIP_TRY(hipMemcpy(c->lw_buf.ptr, w_host, (size_t)bytes, hipMemcpyHostToDevice));
  }
  c->lw_sets = w_host ? nsets : 0;
  c->w.lw = LossW{};
  for (auto& x : c->lw_count) x = 0;
  return SMAML_OK;
}

int smaml_set_score_weights(smaml_ctx* c, const float* node_w_host) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  if (node_w_host) {
    TRY(check_weights(node_w_host, c->d.N, "score weights:"));
    TRY(ensure_device(c));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(c->sw_buf.grow((int64_t)c->d.N * 4));
    HIP_TRY(hipMemcpy(c->sw_buf.ptr, node_w_host, (size_t)c->d.N * 4, hipMemcpyHostToDevice));
  }
  c->sw_set = node_w_host != nullptr;
  for (auto& x : c->lw_count) x = 0;
  return SMAML_OK;
}

int smaml_loss_stats(const smaml_ctx* c, int64_t* counts, int32_t cap, int32_t* count) {
  if (!c || cap < 0 || (cap > 0 && !counts)) return fail(SMAML_EINVAL, "bad loss_stats arguments");
  const int64_t v[6] = {c->lw_sets, c->sw_set ? 1 : 0, c->lw_count[0], c->lw_count[1], c->lw_count[2], c->lw_count[3]};
  for (int i = 0; i < 6 && i < cap; ++i) counts[i] = v[i];
  if (count) *count = 6;
  return SMAML_OK;
}

int smaml_set_gcn_params(smaml_ctx* c, const float* gcn_flat) {
  if (!c || !gcn_flat) return fail(SMAML_EINVAL, "NULL argument");
  if (!aligned16(gcn_flat)) return fail(SMAML_EINVAL, "gcn params must be 16-byte aligned");
  c->gcn = gcn_flat;
  ad_cache_invalidate(c);  // cached features belong to the previous GCN parameters (the slots stay allocated)
  gc_invalidate(c);     // (parameters may be rewritten in place behind a kept pointer: the call is the signal)
  return SMAML_OK;
}

int smaml_gcn_cache_invalidate(smaml_ctx* c) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  gc_invalidate(c);
  return SMAML_OK;
}

int smaml_reserve(smaml_ctx* c, int32_t tasks, int32_t batch) {
  if (!c || tasks <= 0 || batch <= 0) return fail(SMAML_EINVAL, "bad reserve arguments");
  TRY(ensure_device(c));
  return reserve(c, tasks, batch);
}

int64_t smaml_workspace_bytes(const smaml_ctx* c) { return c ? c->arena.cap : 0; }

int32_t smaml_so_kept_steps(const smaml_ctx* c) { return c ? c->keep_last : 0; }

int smaml_set_dropout(smaml_ctx* c, float p_gcn, float p_lstm, uint32_t seed) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  if (!(p_gcn >= 0.f && p_gcn < 1.f) || !(p_lstm >= 0.f && p_lstm < 1.f))
    return fail(SMAML_EINVAL, "dropout probabilities must lie in [0, 1)");
  c->p_gcn = p_gcn;
  c->p_lstm = p_lstm;
  c->drop_seed = seed;
  return SMAML_OK;
}

int smaml_set_task_ids(smaml_ctx* c, const int32_t* ids_host, int32_t n) {
  if (!c || n < 0 || (n > 0 && !ids_host)) return fail(SMAML_EINVAL, "bad set_task_ids arguments");
  c->task_ids.assign(ids_host, ids_host + n);
  return SMAML_OK;
}

// The graph entry points gather rows 0 .. num_nodes - 1 of x into the t = 0 block: an x with fewer rows than the
// graph has nodes would be read past its end (PyG raises an IndexError there).
static int check_gcn_rows(const smaml_ctx* c, int32_t rows, const char* who) {
  if (rows < c->d.N)
    return fail(SMAML_EINVAL, std::string(who) + ": rows (" + std::to_string(rows) + ") must be at least num_nodes (" +
                                  std::to_string(c->d.N) + ") unless SMAML_GCN_PLAIN: the t = 0 block gathers rows 0 .. "
                                  "num_nodes - 1 of x");
  return SMAML_OK;
}

int smaml_gcn_conv(smaml_ctx* c, void* stream, const float* x, int32_t rows, int32_t cin, const float* weight,
                   const float* bias, int32_t cout, float* out) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  if (!graph_set(c)) return fail(SMAML_ESTATE, "smaml_set_graph not called");
  if (!x || !weight || !bias || !out || rows <= 0 || cin <= 0 || cout <= 0)
    return fail(SMAML_EINVAL, "bad gcn_conv arguments");
  if (cin % 4) return fail(SMAML_EINVAL, "cin must be a multiple of 4");
  if (!aligned16(x) || !aligned16(weight)) return fail(SMAML_EINVAL, "x / weight must be 16-byte aligned");
  TRY(check_gcn_rows(c, rows, "smaml_gcn_conv"));
  TRY(ensure_device(c));
  hipStream_t s = (hipStream_t)stream;
  launch_gcn_layer(s, c->d, 0, 1, 1, nullptr, x, out, false, false, weight, bias, cin, cout,
                   graph_view(c), rows, c->d.N);
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_gcn_conv_ex(smaml_ctx* c, void* stream, const float* x, int32_t rows, int32_t cin, const float* weight,
                      const float* bias, int32_t cout, int32_t flags, float* out) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  const bool plain = (flags & SMAML_GCN_PLAIN) != 0, relu = (flags & SMAML_GCN_RELU) != 0;
  if (!plain && !graph_set(c)) return fail(SMAML_ESTATE, "smaml_set_graph not called");
  if (!x || !weight || !bias || !out || rows <= 0 || cin <= 0 || cout <= 0 || (flags & ~3))
    return fail(SMAML_EINVAL, "bad gcn_conv_ex arguments");
  if (cin % 4) return fail(SMAML_EINVAL, "cin must be a multiple of 4");
  if (!aligned16(x) || !aligned16(weight)) return fail(SMAML_EINVAL, "x / weight must be 16-byte aligned");
  if (!plain) TRY(check_gcn_rows(c, rows, "smaml_gcn_conv_ex"));
  TRY(ensure_device(c));
  TRY(check_device_error(c));
  hipStream_t s = (hipStream_t)stream;
  launch_gcn_layer(s, c->d, 0, 1, 1, nullptr, x, out, false, relu, weight, bias, cin, cout,
                   graph_view(c), rows, plain ? 0 : c->d.N);
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_gcn_conv_backward(smaml_ctx* c, void* stream, const float* x, int32_t rows, int32_t cin,
                            const float* weight, int32_t cout, const float* dz, int32_t flags, float* dx, float* dwb) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  const bool plain = (flags & SMAML_GCN_PLAIN) != 0;
  if (!plain && !graph_set(c)) return fail(SMAML_ESTATE, "smaml_set_graph not called");
  if (!x || !weight || !dz || rows <= 0 || cin <= 0 || cout <= 0 || (flags & ~SMAML_GCN_PLAIN) || (!dx && !dwb))
    return fail(SMAML_EINVAL, "bad gcn_conv_backward arguments");
  if (cin % 4 || cout % 4) return fail(SMAML_EINVAL, "cin and cout must be multiples of 4");
  if (!aligned16(x) || !aligned16(weight) || !aligned16(dz) || (dx && !aligned16(dx)))
    return fail(SMAML_EINVAL, "x / weight / dz / dx must be 16-byte aligned");
  if (!plain) TRY(check_gcn_rows(c, rows, "smaml_gcn_conv_backward"));
  TRY(ensure_device(c));
  TRY(check_device_error(c));
  TRY(reserve(c, 1, 1));  // the split-K partial slabs of the weight gradient
  hipStream_t s = (hipStream_t)stream;
  const int ng = plain ? 0 : c->d.N;
  TRY(gcn_conv_bwd(c, s, x, rows, rows, cin, weight, cout, dz, ng, dx, dwb, 0, (int64_t)cout * cin));
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_relu_mask(smaml_ctx* c, void* stream, float* g, const float* h, int64_t n) {
  if (!c || !g || !h || n <= 0) return fail(SMAML_EINVAL, "bad relu_mask arguments");
  TRY(ensure_device(c));
  launch_relu_mask((hipStream_t)stream, g, h, n);
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_forward(smaml_ctx* c, void* stream, const float* theta, const float* const* x_host, int32_t nsamples,
                  float* pred, float* feats) {
  TRY(require_ready(c));
  TRY(check_lstm_dims(c->dims, "smaml_forward"));
  if (!theta || !x_host || nsamples <= 0 || !pred) return fail(SMAML_EINVAL, "bad forward arguments");
  for (int i = 0; i < nsamples; ++i)
    if (!x_host[i] || !aligned16(x_host[i])) return fail(SMAML_EINVAL, "sample x pointers must be 16-B aligned");
  TRY(ensure_device(c));
  hipStream_t s = (hipStream_t)stream;
  TRY(reserve(c, 1, nsamples));
  set_work(c, 1, nsamples);
  TRY(upload_xtab(c, s, x_host, nsamples));
  const float* const* xt = nullptr;
  TRY(xtab_at(c, 0, &xt));
  if (c->p_gcn > 0.f || c->p_lstm > 0.f) {  // train-mode module forward: masks of (seed, task id, step 0)
    TRY(upload_task_ids(c, s, 1));
    set_step_drop(c, 0);  // kept in c->w.drop for the smaml_backward of these activations
  }
  TRY(run_forward(c, s, theta, 0, xt));
  Work w = c->w;
  w.pred = pred;
  launch_head_loss(s, c->d, w, theta, 0, c->po, nullptr, 0.f, false);
  c->act_B = nsamples;
  if (feats) {
    const Dims& d = c->d;
    const int64_t blk = (int64_t)d.N * d.Hc;
    for (int si = 0; si < nsamples; ++si) {
      // F is [T][M][Hc] with M = nsamples*N; feats is [s][T*N][Hc]
      HIP_TRY(hipMemcpy2DAsync(feats + (int64_t)si * d.T * blk, blk * 4, c->w.F + (int64_t)si * blk,
                               (int64_t)nsamples * blk * 4, blk * 4, d.T, hipMemcpyDeviceToDevice, s));
    }
  }
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_set_tasks(smaml_ctx* c, int32_t ntasks, const float* const* features_host, const int32_t* t_total_host) {
  if (c) ad_cache_invalidate(c);
  if (!c || ntasks <= 0 || !features_host || !t_total_host) return fail(SMAML_EINVAL, "bad set_tasks arguments");
  c->feats.assign(features_host, features_host + ntasks);
  c->t_total.assign(t_total_host, t_total_host + ntasks);
  for (int j = 0; j < ntasks; ++j) {
    if (!c->feats[j] || !aligned16(c->feats[j])) return fail(SMAML_EINVAL, "feature streams must be 16-B aligned");
    if (c->t_total[j] < c->d.T + c->d.Hf + 1) return fail(SMAML_EINVAL, "feature stream shorter than one sample");
  }
  return SMAML_OK;
}

int smaml_forecast(smaml_ctx* c, void* stream, const float* theta, int32_t task, const int32_t* windows_host,
                   int32_t nwin, int32_t batch, const float* scale_host, float* pred, double* skill) {
  ForecastCall a;
  a.name = "smaml_forecast";
  a.no_output = "pred and skill are both NULL (nothing to compute)";
  a.any_output = pred || skill;
  a.theta = theta;
  a.list = windows_host;
  a.n = nwin;
  a.batch = batch;
  a.task = task;
  a.score = skill != nullptr;
  a.scale_host = scale_host;
  TRY(forecast_check(c, a));
  hipStream_t s = (hipStream_t)stream;
  const int64_t per = (int64_t)c->d.N * c->d.HfC;  // floats of one window's prediction
  return forecast_run(c, s, a, window_ptrs(c, a), [&](int64_t done, int B, const float* scale_dev) -> int {
    const float* const* xt = nullptr;
    TRY(xtab_at(c, done, &xt));
    return forecast_pass(c, s, theta, xt, B, windows_consec(windows_host + done, B), pred ? pred + done * per : nullptr,
                         scale_dev, skill, done == 0);
  });
}

int64_t smaml_forecast_bytes(const smaml_ctx* c) {
  if (!c) return 0;
  return c->fc_ring.cap + c->fc_F.cap + c->fc_gcnA.cap + c->fc_gcnB.cap + c->fc_xg.cap + c->fc_pred.cap +
         c->fc_part.cap + c->fc_scale.cap + c->ens_ring.cap + c->ens_pred.cap + c->ro_seq.cap + c->ro_xg.cap +
         c->ro_F0.cap + c->ro_blk.cap + c->re_seq.cap + c->re_xg.cap + c->re_obs.cap + c->re_F0.cap + c->re_traj.cap;
}

int smaml_forecast_rollout(smaml_ctx* c, void* stream, const float* theta, int32_t task, const int32_t* origins_host,
                           int32_t norig, int32_t batch, int32_t cycles, int32_t gap, const float* scale_host,
                           float* traj, double* skill) {
  ForecastCall a;
  a.name = "smaml_forecast_rollout";
  a.no_output = "traj and skill are both NULL (nothing to compute)";
  a.any_output = traj || skill;
  a.theta = theta;
  a.list = origins_host;
  a.n = norig;
  a.batch = batch;
  a.task = task;
  a.score = skill != nullptr;
  a.scale_host = scale_host;
  a.rollout = true;
  a.cycles = cycles;
  a.gap = gap;
  TRY(forecast_check(c, a));
  hipStream_t s = (hipStream_t)stream;
  const Dims& d = c->d;
  const int sl = d.Hf + 1, R = cycles;
  RollPlan p = roll_plan(c, a);
  const int Bmax = p.Bmax;
  // every buffer at the largest pass's size before the first launch, so no table entry can dangle
  const int64_t Mx = (int64_t)Bmax * d.N, seq_rows = roll_seq_rows(d, R), nrun_max = std::max(d.T - 1, 1);
  const int64_t grows = p.fused ? Mx : nrun_max * Mx;
  if (c->ro_seq.grow(Bmax * seq_rows * d.N * d.Cin0 * 4) != hipSuccess ||
      c->ro_xg.grow((int64_t)(p.S + 1) * Mx * 4 * d.H * 4) != hipSuccess ||
      c->ro_F0.grow(Mx * d.Hc * 4) != hipSuccess || c->fc_F.grow(nrun_max * Mx * d.Hc * 4) != hipSuccess ||
      grow_all<HipAlloc>({{&c->fc_gcnA, grows * d.Hc * 4}, {&c->fc_gcnB, grows * d.Hc * 4}}) != hipSuccess ||
      c->fc_ring.grow(2 * infer_ring_floats(d, 1, (int)Mx) * 4) != hipSuccess ||
      c->fc_pred.grow(Mx * d.HfC * 4) != hipSuccess ||
      (!traj && c->ro_blk.grow((int64_t)Bmax * sl * d.N * d.C * 4) != hipSuccess) ||
      (skill && c->fc_part.grow((int64_t)rollout_skill_blocks(d, Bmax) * sl * d.C * 3 * 4) != hipSuccess) ||
      (p.fused && c->gcn_wimg.grow(gcn_wimg_bytes(d)) != hipSuccess))
    return fail(SMAML_ENOMEM, "hipMalloc of the rollout buffers failed (batch " + std::to_string(Bmax) + ", " +
                                  std::to_string(R) + " cycles)");
  const std::vector<const float*> ptrs = roll_table(c, a, c->ro_seq.as<float>(), p);
  for (auto& x : c->ro_stats) x = 0;
  return forecast_run(c, s, a, ptrs, [&](int64_t done, int B, const float* scale_dev) -> int {
    return rollout_pass(c, s, a, p, done, B, scale_dev, traj, skill);
  });
}

int smaml_rollout_stats(const smaml_ctx* c, int64_t* counts, int32_t cap, int32_t* count) {
  if (!c || cap < 0 || (cap > 0 && !counts)) return fail(SMAML_EINVAL, "bad rollout_stats arguments");
  for (int i = 0; i < 5 && i < cap; ++i) counts[i] = c->ro_stats[i];
  if (count) *count = 5;
  return SMAML_OK;
}

int smaml_forecast_rollout_ensemble(smaml_ctx* c, void* stream, const float* theta, int32_t task,
                                    const int32_t* origins_host, int32_t norig, int32_t batch, int32_t cycles,
                                    int32_t gap, int32_t members, float p_gcn, float p_lstm, uint32_t seed,
                                    const float* scale_host, float* member_traj, float* mean, float* spread,
                                    double* scores) {
  ForecastCall a;
  a.name = "smaml_forecast_rollout_ensemble";
  a.no_output = "member_traj, mean, spread and scores are all NULL (nothing to compute)";
  a.any_output = member_traj || mean || spread || scores;
  a.theta = theta;
  a.list = origins_host;
  a.n = norig;
  a.batch = batch;
  a.task = task;
  a.score = scores != nullptr;
  a.scale_host = scale_host;
  a.rollout = true;
  a.cycles = cycles;
  a.gap = gap;
  a.ens = true;
  a.members = members;
  a.p_gcn = p_gcn;
  a.p_lstm = p_lstm;
  a.seed = seed;
  TRY(forecast_check(c, a));
  hipStream_t s = (hipStream_t)stream;
  const Dims& d = c->d;
  const int sl = d.Hf + 1, R = cycles, E = members;
  const bool shared = p_gcn == 0.f;
  RollPlan p = roll_plan(c, a);
  const int Bmax = p.Bmax;
  // members per launch set: option ens_group, else as many as fit the budget (at least one)
  if (c->ens_group > 0) p.G = std::min(c->ens_group, E);
  else if (c->ens_group == 0) p.G = E;
  else
    p.G = (int)std::max<int64_t>(
        1, std::min<int64_t>(E, (c->roll_ens_budget_mb << 20) / rens_member_bytes(d, Bmax, R, !shared)));
  const int G = p.G;
  // every buffer at the largest pass's and group's size before the first launch, so no table entry can dangle
  const int64_t Mx = (int64_t)Bmax * d.N, seq_rows = roll_seq_rows(d, R), nrun_max = std::max(d.T - 1, 1);
  const int64_t blkf = (int64_t)sl * d.N * d.C;
  // (the per-layer chain's ping-pong buffers: a chunk of samples below 2^28 floats, or one member's T-row window)
  const int64_t crows = p.fused ? 1 : nrun_max;  // (the fused stack takes the runs: only the t = 0 rows chain)
  const int64_t chain = shared ? std::min<int64_t>((int64_t)G * Mx * crows * d.Hc,
                                                   std::max<int64_t>(1ll << 28, crows * d.N * d.Hc))
                               : (int64_t)d.T * Mx * d.Hc;
  if (c->re_seq.grow((int64_t)G * Bmax * seq_rows * d.N * d.Cin0 * 4) != hipSuccess ||
      (shared && c->re_xg.grow((int64_t)(p.S + 1) * G * Mx * 4 * d.H * 4) != hipSuccess) ||
      (shared && c->re_obs.grow((int64_t)(d.T + 1) * Mx * 4 * d.H * 4) != hipSuccess) ||
      (shared && c->re_F0.grow((int64_t)G * Mx * d.Hc * 4) != hipSuccess) ||
      c->fc_F.grow((shared ? nrun_max : (int64_t)d.T) * G * Mx * d.Hc * 4) != hipSuccess ||
      grow_all<HipAlloc>({{&c->fc_gcnA, chain * 4}, {&c->fc_gcnB, chain * 4}}) != hipSuccess ||
      c->ens_ring.grow(2 * infer_ring_floats(d, G, (int)Mx) * 4) != hipSuccess ||
      c->ens_pred.grow((int64_t)G * Mx * d.HfC * 4) != hipSuccess ||
      (!member_traj && c->re_traj.grow((int64_t)E * Bmax * R * blkf * 4) != hipSuccess) ||
      (scores && c->fc_part.grow((int64_t)skill_blocks(d, Bmax) * R * sl * d.C * 4 * 4) != hipSuccess) ||
      (shared && p.fused && c->gcn_wimg.grow(gcn_wimg_bytes(d)) != hipSuccess))
    return fail(SMAML_ENOMEM, "hipMalloc of the ensemble-rollout buffers failed (batch " + std::to_string(Bmax) + ", " +
                                  std::to_string(R) + " cycles, " + std::to_string(G) + " members at a time)");
  const std::vector<const float*> ptrs = roll_table(c, a, c->re_seq.as<float>(), p);
  for (auto& x : c->re_stats) x = 0;
  return forecast_run(c, s, a, ptrs, [&](int64_t done, int B, const float* scale_dev) -> int {
    return rens_pass(c, s, a, p, done, B, scale_dev, member_traj, mean, spread, scores);
  });
}

int smaml_rollout_ensemble_stats(const smaml_ctx* c, int64_t* counts, int32_t cap, int32_t* count) {
  if (!c || cap < 0 || (cap > 0 && !counts)) return fail(SMAML_EINVAL, "bad rollout_ensemble_stats arguments");
  for (int i = 0; i < 7 && i < cap; ++i) counts[i] = c->re_stats[i];
  if (count) *count = 7;
  return SMAML_OK;
}

int smaml_forecast_ensemble(smaml_ctx* c, void* stream, const float* theta, int32_t task, const int32_t* windows_host,
                            int32_t nwin, int32_t batch, int32_t members, float p_gcn, float p_lstm, uint32_t seed,
                            const float* scale_host, float* mean, float* spread, float* member_pred, double* scores) {
  ForecastCall a;
  a.name = "smaml_forecast_ensemble";
  a.no_output = "mean, spread, member_pred and scores are all NULL";
  a.any_output = mean || spread || member_pred || scores;
  a.theta = theta;
  a.list = windows_host;
  a.n = nwin;
  a.batch = batch;
  a.task = task;
  a.score = scores != nullptr;
  a.scale_host = scale_host;
  a.ens = true;
  a.members = members;
  a.p_gcn = p_gcn;
  a.p_lstm = p_lstm;
  a.seed = seed;
  TRY(forecast_check(c, a));
  hipStream_t s = (hipStream_t)stream;
  const int64_t per = (int64_t)c->d.N * c->d.HfC;
  return forecast_run(c, s, a, window_ptrs(c, a), [&](int64_t done, int B, const float* scale_dev) -> int {
    const float* const* xt = nullptr;
    TRY(xtab_at(c, done, &xt));
    const int64_t off = done * per;
    return ensemble_pass(c, s, theta, xt, B, windows_consec(windows_host + done, B), a, done, scale_dev,
                         mean ? mean + off : nullptr, spread ? spread + off : nullptr,
                         member_pred ? member_pred + off : nullptr, scores);
  });
}

// One meta-step as its entry point received it (smaml_meta_step; smaml_meta_step_base: gcn_meta_grad set).
struct MetaCall {
  const float* theta;
  int order, steps, batch;
  const int32_t* windows;
  float inner_lr, max_norm, query_scale;
  float *meta_grad, *gcn_meta_grad, *losses, *norms, *fast_out;
};

// The buffers of smaml_meta_step_base's base stage (mb_buf) for steps of Z tasks and B windows.
struct MbBufs {
  float *dz = nullptr, *h[3] = {}, *gn = nullptr, *xcat = nullptr, *S = nullptr, *RS = nullptr;
  float *part = nullptr, *acc = nullptr;  // [Z][2][Pg] the stage's blocks, [Z][Pg] the call's sum
  int64_t rows = 0;                       // B*T*N: the rows of a task in the per-sample form (the larger one)
};

// Every buffer of the base stage before the call's first launch: a failure leaves the outputs untouched.
static int mb_prepare(smaml_ctx* c, int Z, int B, MbBufs* mb) {
  const Dims& d = c->d;
  const int64_t rows = (int64_t)B * d.T * d.N, Pg = c->go.total;
  if (rows * std::max(d.Hc, 8 * d.H) >= (1ll << 31))
    return fail(SMAML_EINVAL, "batch too large: B*T*N*max(Hc, 8H) must stay below 2^31");
  const int64_t hsz = rows * d.Hc, xsz = rows * d.Cin0, ssz = (int64_t)Z * xg_dedup_rows(B, d.T, d.N) * 4 * d.H;
  const int64_t total = (int64_t)Z * hsz + 4 * hsz + xsz + 2 * ssz + 3 * (int64_t)Z * Pg;
  if (c->mb_buf.grow(total * 4) != hipSuccess ||
      c->bw_scratch.grow(2 * rows * std::max(d.Hc, d.Cin0) * 4) != hipSuccess)
    return fail(SMAML_ENOMEM, "smaml_meta_step_base: hipMalloc of the base stage's buffers failed (nothing was launched)");
  float* p = c->mb_buf.as<float>();
  mb->rows = rows;
  mb->dz = p, p += (int64_t)Z * hsz;
  for (int l = 0; l < 3; ++l) mb->h[l] = p, p += hsz;
  mb->gn = p, p += hsz;
  mb->xcat = p, p += xsz;
  mb->S = p, p += ssz;
  mb->RS = p, p += ssz;
  mb->part = p, p += 2 * (int64_t)Z * Pg;
  mb->acc = p;
  for (auto& x : c->mb_stats) x = 0;
  c->mb_stats[4] = c->mb_buf.cap;
  return SMAML_OK;
}

// The base stage of one step of smaml_meta_step_base, right after the step's run_backward (U null) or
// run_backward_dual (U = the sweep direction): acc[z] += alpha * d(.)/dg of task z, from layer 0's gate gradients
// (w.dG; tangent: w.RGs too) through W_ih0 (th + z P; tangent: U's block too), conv4's ReLU (the features the
// step's forward read, w.F) and conv4..conv1 with conv1..conv3's outputs recomputed from the step's windows.
//   distinct-row form (the step's tasks read consecutive windows, wgrad_dedup_ok, option meta_base_dedup): per
//     task the B N rows of t = 0 as B samples of N rows on the graph path, then stream rows w0 + 1 .. w0 + B + T - 2
//     as one neighbour-less block; both are slices of the stream (first[z] = the task's first window), the
//     gradient rows are k_dg_rowsum's sums (the mask and the sum over a stream row's slots commute).
//   per-sample form: B samples of T N rows in smaml_backward_base's layout (xt = the step's window table).
// Each block's dW, db go to a slot of its own; the slots are added in task and block order.
static int meta_base_stage(smaml_ctx* c, hipStream_t s, const MbBufs& mb, const float* const* xt,
                           const float* const* first, const float* th, const float* U, float alpha) {
  const Dims& d = c->d;
  Work& w = c->w;
  const int Z = w.Z, B = w.B, M = w.M, G4 = 4 * d.H;
  const int64_t TM = (int64_t)d.T * M, P = c->po.P, Pg = c->go.total, hz = mb.rows * d.Hc;
  const bool distinct = c->meta_base_dedup && wgrad_dedup_ok(c);
  const GraphView gv = graph_view(c);
  Dx0Meta a;
  a.W = th + c->po.lay[0].wih;
  a.U = U ? U + c->po.lay[0].wih : nullptr;
  a.w_zstride = P;
  a.F = w.F;
  a.f_zstride = TM * d.Hc;
  a.out = mb.dz;
  a.o_zstride = hz;
  a.K = G4, a.Hc = d.Hc, a.T = d.T, a.M = M, a.N = d.N;
  a.mdiv = FastDiv((uint32_t)M), a.ndiv = FastDiv((uint32_t)d.N);
  a.fcompact = w.fcompact;
  a.distinct = distinct ? 1 : 0;
  const int rows1 = d.T > 1 ? (B + d.T - 2) * d.N : 0;  // the stream rows past t = 0 (none at T = 1)
  if (distinct && d.T > 1) {
    const int64_t sz = xg_dedup_rows(B, d.T, d.N) * G4;
    TIMED(c, s, C_DGSUM, 0, launch_dg_rowsum(s, d, w, w.dG, TM * G4, mb.S));
    if (U) TIMED(c, s, C_DGSUM, 0, launch_dg_rowsum(s, d, w, w.RGs, TM * G4, mb.RS));
    a.A = mb.S, a.RA = U ? mb.RS : nullptr, a.a_zstride = sz;
    a.rows = M + rows1;
  } else {  // every slot row (distinct at T = 1: the t = 0 rows are all there is)
    a.A = w.dG, a.RA = U ? w.RGs : nullptr, a.a_zstride = TM * G4;
    a.rows = (int)TM;
  }
  TIMED(c, s, C_MISC, 2.0 * Z * a.rows * (U ? 2 : 1) * G4 * d.Hc, launch_lstm_dx0_meta(s, a, Z));
  // one block of rows: conv1..conv3 recomputed, then conv4 -> conv1 into the block's slot
  auto block = [&](const float* const* tab, const float* x0, int nsamp, int rps, int ng, int64_t row0) -> int {
    const int rows = nsamp * rps;
    float* h[3];
    for (int l = 0; l < 3; ++l) h[l] = mb.h[l] + row0 * d.Hc;
    for (int l = 0; l < 3; ++l)
      TIMED(c, s, C_GCN, 2.0 * rows * c->go.cin[l] * d.Hc,
            launch_gcn_layer(s, d, l, nsamp, nsamp, l == 0 ? tab : nullptr, l == 0 ? (tab ? nullptr : x0) : h[l - 1], h[l],
                             false, true, c->gcn + c->go.w[l], c->gcn + c->go.b[l], c->go.cin[l], d.Hc, gv, rps, ng,
                             nullptr));
    return SMAML_OK;
  };
  for (int z = 0; z < Z; ++z) {
    float* slot = mb.part + (int64_t)z * 2 * Pg;
    float *g = mb.dz + (int64_t)z * hz, *gn = mb.gn;
    int nblk = 1;
    if (distinct) {
      const float* x0 = first[z];
      float* h0[3] = {mb.h[0], mb.h[1], mb.h[2]};
      TRY(block(nullptr, x0, B, d.N, d.N, 0));
      TRY(gcn_backward_chain(c, s, x0, h0, g, gn, M, d.N, c->gcn, slot, false, nullptr, nullptr, C_GCN));
      if (rows1 > 0) {
        const float* x1 = x0 + (int64_t)d.N * d.Cin0;
        float* h1[3] = {mb.h[0] + (int64_t)M * d.Hc, mb.h[1] + (int64_t)M * d.Hc, mb.h[2] + (int64_t)M * d.Hc};
        float *g1 = mb.dz + (int64_t)z * hz + (int64_t)M * d.Hc, *gn1 = mb.gn + (int64_t)M * d.Hc;
        TRY(block(nullptr, x1, 1, rows1, 0, M));
        TRY(gcn_backward_chain(c, s, x1, h1, g1, gn1, rows1, rows1, c->gcn, slot + Pg, false, nullptr, nullptr, C_GCN, 0));
        nblk = 2;
      }
      c->mb_stats[5] += M + rows1;
    } else {
      const int rps = d.T * d.N;
      float* h0[3] = {mb.h[0], mb.h[1], mb.h[2]};
      TIMED(c, s, C_GCN, 0, launch_gather_slabs(s, xt + (int64_t)z * B, B, (int64_t)rps * d.Cin0, mb.xcat));
      TRY(block(xt + (int64_t)z * B, nullptr, B, rps, d.N, 0));
      TRY(gcn_backward_chain(c, s, mb.xcat, h0, g, gn, B * rps, rps, c->gcn, slot, false, nullptr, nullptr, C_GCN));
      c->mb_stats[5] += (int64_t)B * rps;
    }
    for (int i = 0; i < nblk; ++i)
      TIMED(c, s, C_MISC, 0, launch_axpy(s, mb.acc + (int64_t)z * Pg, slot + (int64_t)i * Pg, Pg, alpha));
  }
  c->mb_stats[0] += 1;
  c->mb_stats[distinct ? 1 : 2] += 1;
  if (U) c->mb_stats[3] += 1;
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

// The meta-step, once: the inner loop, the query step and (order 2) the sweep; with a.gcn_meta_grad the base
// stage after the query step's backward and after each sweep step's tangent backward. The launches of a call
// without it are smaml_meta_step's, in its order.
static int meta_run(smaml_ctx* c, hipStream_t s, const MetaCall& a) {
  const float* theta = a.theta;
  const int order = a.order, steps = a.steps, batch = a.batch;
  const int32_t* windows_host = a.windows;
  const float inner_lr = a.inner_lr, max_norm = a.max_norm, query_scale = a.query_scale;
  float *meta_grad = a.meta_grad, *losses = a.losses, *norms = a.norms, *fast_out = a.fast_out;
  const bool base = a.gcn_meta_grad != nullptr;
  TRY(ensure_device(c));
  const Dims& d = c->d;
  const int Z = (int)c->feats.size();
  const int B = batch;
  TRY(ensure_bar(c));
  TRY(check_device_error(c));
  TRY(reserve(c, Z, B, order == 2));
  // sample window table for every step (support steps then the query batch)
  const int64_t nptr = (int64_t)(steps + 1) * Z * B;
  // (+ each step's per-task first-window pointers, the GCN's consecutive-window tables)
  std::vector<const float*> ptrs(nptr + (int64_t)(steps + 1) * Z);
  const int max_w_off = d.T + d.Hf;  // last stream index read by a sample = w + T + Hf
  for (int k = 0; k <= steps; ++k)
    for (int z = 0; z < Z; ++z)
      for (int b = 0; b < B; ++b) {
        const int64_t i = ((int64_t)k * Z + z) * B + b;
        const int wv = windows_host[i];
        if (wv < 0 || wv + max_w_off >= c->t_total[z])
          return fail(SMAML_EINVAL, "window start out of range for task " + std::to_string(z));
        ptrs[i] = c->feats[z] + (int64_t)wv * d.N * d.Cin0;
      }
  // steps whose every task reads B consecutive windows (the reference's support and query batches)
  std::vector<char> is_consec(steps + 1, 0);
  for (int k = 0; k <= steps; ++k) {
    bool ok = B > 1;
    for (int z = 0; z < Z && ok; ++z) {
      const int32_t* wz = windows_host + ((int64_t)k * Z + z) * B;
      for (int b = 1; b < B && ok; ++b) ok = wz[b] == wz[0] + b;
    }
    for (int z = 0; z < Z; ++z) ptrs[nptr + (int64_t)k * Z + z] = ptrs[((int64_t)k * Z + z) * B];
    is_consec[k] = ok;
  }
  // The per-stream GCN feature cache serves the consecutive-window steps when every task of the group has its
  // tables (gc_prepare; they do not move before this call returns): behind the tables above, per such step and
  // task, where its first window starts in t0 and one stream row later in t1 (launch_gcn_cache_gather).
  std::vector<smaml_ctx::GcEntry*> gc_ent;
  std::vector<int32_t> gc_w0((size_t)(steps + 1) * Z, 0);
  struct GcScope {  // the step views point into this call's vectors
    smaml_ctx* c;
    ~GcScope() { c->gc_cur = {}; }
  } gc_scope{c};
  const bool any_consec = std::find(is_consec.begin(), is_consec.end(), (char)1) != is_consec.end();
  const bool gc_use = c->gc_on && c->kn.gcn_dedup && c->p_gcn == 0.f && any_consec && gc_prepare(c, Z, gc_ent);
  const int64_t gc_base = (int64_t)ptrs.size();
  if (gc_use) {
    ptrs.resize((size_t)gc_base + (size_t)(steps + 1) * Z * 2, nullptr);
    const int64_t blk = (int64_t)d.N * d.Hc;
    for (int k = 0; k <= steps; ++k)
      for (int z = 0; z < Z && is_consec[k]; ++z) {
        const int32_t w0 = windows_host[((int64_t)k * Z + z) * B];
        const float* t0 = gc_ent[z]->tab.as<float>();
        gc_w0[(size_t)k * Z + z] = w0;
        ptrs[gc_base + ((int64_t)k * Z + z) * 2] = t0 + (int64_t)w0 * blk;
        ptrs[gc_base + ((int64_t)k * Z + z) * 2 + 1] = t0 + ((int64_t)gc_ent[z]->t_total + w0 + 1) * blk;
      }
  }
  // every support step served from the cache: the sweep takes its features there too, no per-step store
  const bool so_cached = gc_use && std::find(is_consec.begin(), is_consec.begin() + steps, (char)0) == is_consec.begin() + steps;
  if (order == 2) TRY(ensure_so_store(c, std::max(steps, 1), Z, B, so_cached));
  if (order == 2) TRY(ensure_keep(c, steps, Z, B, so_cached));
  MbBufs mb;
  if (base) TRY(mb_prepare(c, Z, B, &mb));
  set_work(c, Z, B);
  use_loss_weights(c, nullptr);  // task z reads set z
  const int nkeep = order == 2 ? std::min(std::min(c->keep_n, c->keep_want), steps) : 0;
  c->keep_last = nkeep;
  TRY(upload_xtab(c, s, ptrs.data(), (int64_t)ptrs.size()));
  // device table pointers per step: windows [k][Z][B] and (consecutive steps) first windows [k][Z]
  std::vector<const float* const*> xstep(steps + 1, nullptr), consec(steps + 1, nullptr), gc_tab(steps + 1, nullptr);
  for (int k = 0; k <= steps; ++k) {
    TRY(xtab_at(c, (int64_t)k * Z * B, &xstep[k]));
    if (is_consec[k]) TRY(xtab_at(c, nptr + (int64_t)k * Z, &consec[k]));
    if (is_consec[k] && gc_use) TRY(xtab_at(c, gc_base + (int64_t)k * Z * 2, &gc_tab[k]));
  }
  // step k's view of the cache (null table: run_gcn computes the step's features itself)
  auto gc_step = [&](int k, bool sweep = false) {
    c->gc_cur.sweep = sweep;
    c->gc_cur.tab = gc_tab[k];
    c->gc_cur.ent = gc_ent.data();
    c->gc_cur.w0 = gc_w0.data() + (size_t)k * Z;
  };
  if (!losses) {
    HIP_TRY(c->scratch_loss.grow((int64_t)(steps + 1) * Z * 4));
    losses = c->scratch_loss.as<float>();
  }
  const int64_t P = c->po.P;
  const float inv = 1.f / ((float)d.N * d.HfC * B);
  const bool dropout = c->p_gcn > 0.f || c->p_lstm > 0.f;
  if (dropout) TRY(upload_task_ids(c, s, Z));
  const int64_t Pg = c->go.total;
  // (the slots' and the sum's pads are zeroed once per call: every stage overwrites the tensors and leaves the pads)
  if (base) HIP_TRY(hipMemsetAsync(mb.part, 0, (size_t)(3 * Z * Pg) * 4, s));
  // each task's first window of step k, as host-side device pointers (the distinct-row form's stream slices)
  auto first_of = [&](int k) { return ptrs.data() + nptr + (int64_t)k * Z; };
  launch_broadcast(s, theta, P, Z, c->fast);
  const double head_fl = 2.0 * Z * c->w.M * d.HfC * d.H;
  const bool so = order == 2;
  float *const so_theta = c->so_theta.as<float>(), *const so_grad = c->so_grad.as<float>();
  float *const so_norm = c->so_norm.as<float>(), *const so_coef = c->so_coef.as<float>();
  float* const so_F = c->so_F.as<float>();
  if (so) c->so_fc.assign((size_t)steps, 0);
  for (int k = 0; k < steps; ++k) {
    const float* const* xt = xstep[k];
    if (dropout) set_step_drop(c, k);
    if (so) {
      HIP_TRY(hipMemcpyAsync(so_theta + (int64_t)k * Z * P, c->fast, (size_t)Z * P * 4, hipMemcpyDeviceToDevice, s));
      c->w.F = so_F ? so_F + (int64_t)k * Z * B * d.T * d.N * d.Hc : c->F_main;
    }
    const int slot = steps - 1 - k;
    use_primal(c, slot < nkeep ? slot : SET_MAIN);
    gc_step(k);
    TRY(run_forward(c, s, c->fast, P, xt, consec[k]));
    if (so) c->so_fc[k] = (int8_t)c->w.fcompact;  // (the layout of so_F slot k, for the sweep)
    TIMED(c, s, C_HEAD, head_fl, launch_head_loss(s, d, c->w, c->fast, P, c->po, xt, 2.f * inv, true));
    TIMED(c, s, C_MISC, 0, launch_loss_final(s, c->w, inv, losses + (int64_t)k * Z));
    TRY(run_backward(c, s, c->fast, P, c->grad));
    // the inner SGD step (clip_grad_norm_ + SGD) of every task: one kernel
    if (so) {
      HIP_TRY(hipMemcpyAsync(so_grad + (int64_t)k * Z * P, c->grad, (size_t)Z * P * 4, hipMemcpyDeviceToDevice, s));
      TIMED(c, s, C_MISC, 0,
            HIP_TRY(launch_inner_sgd(s, c->fast, c->grad, P, Z, c->w.sqpart, inner_lr, max_norm,
                                     so_norm + (int64_t)k * Z, so_coef + (int64_t)k * Z, bar_plan(c))));
      if (norms)
        HIP_TRY(hipMemcpyAsync(norms + (int64_t)k * Z, so_norm + (int64_t)k * Z, Z * 4, hipMemcpyDeviceToDevice, s));
    } else {
      TIMED(c, s, C_MISC, 0,
            HIP_TRY(launch_inner_sgd(s, c->fast, c->grad, P, Z, c->w.sqpart, inner_lr, max_norm,
                                     norms ? norms + (int64_t)k * Z : nullptr, nullptr, bar_plan(c))));
    }
  }
  const float* const* xq = xstep[steps];
  c->w.F = c->F_main;
  use_primal(c, nkeep > 0 ? SET_QUERY : SET_MAIN);  // slot 0 holds the workspace's own Hs/Cs/Gs
  if (dropout) set_step_drop(c, steps);
  gc_step(steps);
  TRY(run_forward(c, s, c->fast, P, xq, consec[steps]));
  TIMED(c, s, C_HEAD, head_fl,
        launch_head_loss(s, d, c->w, c->fast, P, c->po, xq, 2.f * inv * query_scale, true));
  TIMED(c, s, C_MISC, 0, launch_loss_final(s, c->w, inv, losses + (int64_t)steps * Z));
  if (order == 1) {
    TRY(run_backward(c, s, c->fast, P, c->grad));
    if (base) TRY(meta_base_stage(c, s, mb, xq, first_of(steps), c->fast, nullptr, 1.f));
    TIMED(c, s, C_MISC, 0, launch_sum_tasks(s, c->grad, P, Z, meta_grad));
  } else if (so) {
    // v_K = d(query_scale * L_q)/d theta_K, then back through every inner step:
    //   v_k = v_{k+1} - lr * H_k w_k,  w_k = clip-adjusted v_{k+1}
    if (fast_out) HIP_TRY(hipMemcpyAsync(fast_out, c->fast, (size_t)Z * P * 4, hipMemcpyDeviceToDevice, s));
    fast_out = nullptr;
    TRY(run_backward(c, s, c->fast, P, c->grad));
    if (base) TRY(meta_base_stage(c, s, mb, xq, first_of(steps), c->fast, nullptr, 1.f));
    use_primal(c, SET_MAIN);
    float* V = c->grad;
    // w_{K-1}: the clip-adjusted direction of the last inner step at v_K (one kernel: dot + direction)
    if (steps > 0)
      TIMED(c, s, C_MISC, 0,
            HIP_TRY(launch_sweep_update(s, V, nullptr, 0.f, so_grad + (int64_t)(steps - 1) * Z * P, P, Z,
                                        c->w.sqpart, so_norm + (int64_t)(steps - 1) * Z,
                                        so_coef + (int64_t)(steps - 1) * Z, max_norm, c->so_u,
                                        bar_plan(c))));
    for (int k = steps - 1; k >= 0; --k) {
      const float* th = so_theta + (int64_t)k * Z * P;
      const float* const* xt = xstep[k];
      c->w.F = so_F ? so_F + (int64_t)k * Z * B * d.T * d.N * d.Hc : c->F_main;
      const int slot = steps - 1 - k;
      use_primal(c, slot < nkeep ? slot : SET_MAIN);
      c->w.primal_kept = slot < nkeep ? 1 : 0;
      if (dropout) set_step_drop(c, k);  // the masks of inner step k's forward
      gc_step(k, true);
      TRY(run_forward_dual(c, s, th, c->so_u, P, xt, so_F != nullptr, consec[k], c->so_fc[k]));
      TIMED(c, s, C_HEAD, 3.0 * head_fl, launch_head_dual(s, d, c->w, th, c->so_u, P, c->po, xt, 2.f * inv));
      TRY(run_backward_dual(c, s, th, c->so_u, P, c->so_hu));
      // the mixed term of step k: -lr d(g_k . w_k)/dg, w_k = so_u (still this step's direction)
      if (base) TRY(meta_base_stage(c, s, mb, xt, first_of(k), th, c->so_u, -inner_lr));
      if (k > 0)  // v_k = v_{k+1} - lr H_k w_k and w_{k-1} (dot g_{k-1} . v_k, direction): one kernel
        TIMED(c, s, C_MISC, 0,
              HIP_TRY(launch_sweep_update(s, V, c->so_hu, -inner_lr, so_grad + (int64_t)(k - 1) * Z * P, P, Z,
                                          c->w.sqpart, so_norm + (int64_t)(k - 1) * Z,
                                          so_coef + (int64_t)(k - 1) * Z, max_norm, c->so_u,
                                          bar_plan(c))));
      else
        TIMED(c, s, C_MISC, 0, launch_axpy(s, V, c->so_hu, (int64_t)Z * P, -inner_lr));
      c->w.primal_kept = 0;
    }
    use_primal(c, SET_MAIN);
    TIMED(c, s, C_MISC, 0, launch_sum_tasks(s, V, P, Z, meta_grad));
    c->w.F = c->F_main;
  }
  if (base) TIMED(c, s, C_MISC, 0, launch_sum_tasks(s, mb.acc, Pg, Z, a.gcn_meta_grad));
  if (fast_out) HIP_TRY(hipMemcpyAsync(fast_out, c->fast, (size_t)Z * P * 4, hipMemcpyDeviceToDevice, s));
  c->w.drop = Drop{};
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_meta_step(smaml_ctx* c, void* stream, const float* theta, int32_t order, int32_t steps, int32_t batch,
                    const int32_t* windows_host, float inner_lr, float max_norm, float query_scale,
                    float* meta_grad, float* losses, float* norms, float* fast_out) {
  TRY(require_ready(c));
  TRY(check_lstm_dims(c->dims, "smaml_meta_step"));
  if (c->feats.empty()) return fail(SMAML_ESTATE, "smaml_set_tasks not called");
  TRY(check_loss_weights(c, "smaml_meta_step"));
  if (!theta || steps < 0 || batch <= 0 || !windows_host) return fail(SMAML_EINVAL, "bad meta_step arguments");
  if (order < 0 || order > 2) return fail(SMAML_EINVAL, "order must be 0, 1 or 2");
  if (order >= 1 && !meta_grad) return fail(SMAML_EINVAL, "meta_grad required for order >= 1");
  return meta_run(c, (hipStream_t)stream,
                  MetaCall{theta, order, steps, batch, windows_host, inner_lr, max_norm, query_scale,
                           meta_grad, nullptr, losses, norms, fast_out});
}

int smaml_meta_step_base(smaml_ctx* c, void* stream, const float* theta, int32_t order, int32_t steps, int32_t batch,
                         const int32_t* windows_host, float inner_lr, float max_norm, float query_scale,
                         float* meta_grad, float* gcn_meta_grad, float* losses, float* norms, float* fast_out) {
  // (the checks that need no context first: they run without a device too)
  if (order != 1 && order != 2)
    return fail(SMAML_EINVAL, "smaml_meta_step_base: order must be 1 or 2 (order 0 has no meta-gradient), got " +
                                  std::to_string(order));
  if (!gcn_meta_grad || !aligned16(gcn_meta_grad))
    return fail(SMAML_EINVAL, "smaml_meta_step_base: gcn_meta_grad must be a 16-byte aligned device pointer");
  if (!theta || steps < 0 || batch <= 0 || !windows_host) return fail(SMAML_EINVAL, "bad meta_step_base arguments");
  if (!meta_grad) return fail(SMAML_EINVAL, "smaml_meta_step_base: meta_grad required");
  TRY(require_ready(c));
  TRY(check_lstm_dims(c->dims, "smaml_meta_step_base"));
  if (c->feats.empty()) return fail(SMAML_ESTATE, "smaml_set_tasks not called");
  TRY(check_loss_weights(c, "smaml_meta_step_base"));
  if (c->p_gcn > 0.f)
    return fail(SMAML_ENOTIMPL, "smaml_meta_step_base: GCN dropout (p_gcn > 0 of smaml_set_dropout) with base "
                                "gradients is not implemented");
  return meta_run(c, (hipStream_t)stream,
                  MetaCall{theta, order, steps, batch, windows_host, inner_lr, max_norm,
                           query_scale, meta_grad, gcn_meta_grad, losses, norms, fast_out});
}

int smaml_meta_base_stats(const smaml_ctx* c, int64_t* counts, int32_t cap, int32_t* count) {
  if (!c || cap < 0 || (cap > 0 && !counts)) return fail(SMAML_EINVAL, "bad meta_base_stats arguments");
  for (int i = 0; i < 6 && i < cap; ++i) counts[i] = c->mb_stats[i];
  if (count) *count = 6;
  return SMAML_OK;
}

// Fill the adaptation feature cache for every window this call reads that it does not hold yet
// (frozen GCN, F2): the missing windows in runs of consecutive starts, each run as ONE GCN pass over
// Z = run-length single-window "tasks" (B = 1), whose [Z][T][N][Hc] output is exactly the run's
// cache slots. Per-row GCN arithmetic does not depend on how many samples a launch holds, so the
// features are bitwise those of the per-step fill (the first epoch no longer runs 960 batch-1 GCNs).
// The windows are those of task `task` (its stream, its cache), windows[i * stride] for i < n.
static int ad_cache_fill(smaml_ctx* c, hipStream_t s, int task, const int32_t* windows, int64_t n, int64_t stride) {
  const Dims& d = c->d;
  const int64_t fsz = (int64_t)d.T * d.N * d.Hc;
  smaml_ctx::AdCache& ac = c->ad[task];
  std::vector<int32_t> need;
  for (int64_t i = 0; i < n; ++i)
    if (!ac.valid[windows[i * stride]]) need.push_back(windows[i * stride]);
  if (need.empty()) return SMAML_OK;
  std::sort(need.begin(), need.end());
  need.erase(std::unique(need.begin(), need.end()), need.end());
  std::vector<const float*> ptrs(need.size());
  for (size_t i = 0; i < need.size(); ++i) ptrs[i] = c->feats[task] + (int64_t)need[i] * d.N * d.Cin0;
  TRY(upload_xtab(c, s, ptrs.data(), (int64_t)ptrs.size()));
  for (size_t i = 0; i < need.size();) {
    size_t j = i + 1;
    while (j < need.size() && need[j] == need[j - 1] + 1 && (int)(j - i) < c->ad_gcn_batch) ++j;
    set_work(c, (int)(j - i), 1);
    c->w.F = ac.F.as<float>() + (int64_t)need[i] * fsz;
    const float* const* xt = nullptr;
    TRY(xtab_at(c, (int64_t)i, &xt));
    TRY(run_gcn(c, s, xt));
    for (size_t k = i; k < j; ++k) ac.valid[need[k]] = 1;
    i = j;
  }
  return SMAML_OK;
}

// Set-up half of smaml_adapt_steps: size the workspace for `B`-sample steps (and, for the batched cache
// fill, ad_gcn_batch single-window "tasks") and allocate the per-window feature cache once per context.
// Both allocations are TOUCHED (memset + stream sync) before returning: the driver may hand out freshly
// released VRAM that it still has to clear, and that clear otherwise lands in the first kernel that
// reads the buffer -- i.e. inside the first timed epoch (round 5: 6.1 s of a 6.8 s first epoch on some
// boxes, 0 on others). Returns with *cache = whether this call's steps use the cache.
// The regions of the call are the `R` tasks `tasks` (smaml_adapt_steps: task 0 alone); the workspace is
// sized for all R as one launch set. Every region gets a cache of its own stream's length, and *cache is
// whether all of them have one (a lockstep step reads all its regions' features the same way).
static int ad_prepare(smaml_ctx* c, hipStream_t s, int B, const int32_t* tasks, int R, bool* cache_out) {
  using clk = std::chrono::steady_clock;
  const Dims& d = c->d;
  auto t0 = clk::now();
  const bool fill_batched = B == 1 && !(c->p_gcn > 0.f) && c->ad_gcn_batch > 1;
  const int64_t had = c->arena.cap;
  // (the cache fill's GCN passes run ad_gcn_batch windows as tasks: size the workspace for them
  // first, since a growing workspace drops the cache)
  if (fill_batched && R < c->ad_gcn_batch) TRY(reserve(c, c->ad_gcn_batch, 1));
  TRY(reserve(c, R, B));
  if (c->arena.cap != had) {
    HIP_TRY(hipMemsetAsync(c->arena.ptr, 0, (size_t)c->arena.cap, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  auto t1 = clk::now();
  const int64_t fsz = (int64_t)d.T * d.N * d.Hc;  // floats of one window's features
  if (c->ad.size() < c->feats.size()) c->ad.resize(c->feats.size());
  bool cache = B == 1 && !(c->p_gcn > 0.f);
  for (int r = 0; r < R && cache; ++r) {
    smaml_ctx::AdCache& ac = c->ad[tasks[r]];
    const int64_t n = c->t_total[tasks[r]];
    if ((int64_t)ac.valid.size() < n) {  // no cache yet, or a longer stream than it was sized for
      ac.valid.clear();
      if (ac.F.grow_if_room(n * fsz * 4, AD_F_MARGIN)) {
        ac.valid.assign((size_t)n, 0);
        HIP_TRY(hipMemsetAsync(ac.F.ptr, 0, (size_t)(n * fsz * 4), s));
        HIP_TRY(hipStreamSynchronize(s));
      }
    }
    cache = ac.F.ptr != nullptr && !ac.valid.empty();
  }
  auto t2 = clk::now();
  c->ad_ph.ms[AD_RESERVE] += std::chrono::duration<double, std::milli>(t1 - t0).count();
  c->ad_ph.ms[AD_ALLOC] += std::chrono::duration<double, std::milli>(t2 - t1).count();
  *cache_out = cache;
  return SMAML_OK;
}

// Regions per launch set of a lockstep call over R regions (option adapt_group; 0 = all at once). The
// default (-1) follows the measurement at config-4 shapes: per region, a set of Z
// regions costs 0.626 ms at Z = 1, 0.60 at 2, 0.80 / 0.65 / 0.66 at 3 / 4 / 5 (the size-based selection
// leaves the one-launch small-grid kernels there, the big tiles are not yet full), 0.60 at 6, 0.49 at 8,
// 0.34 at 18 -- so 3 to 5 regions run in sets of 2, every other count all at once.
static int ad_group_size(const smaml_ctx* c, int R) {
  if (c->ad_group > 0) return std::min(c->ad_group, R);
  if (c->ad_group < 0 && R >= 3 && R <= 5) return 2;
  return std::min(R, ADAPT_MAX_GROUP);
}

// The regions of a lockstep call: distinct tasks of smaml_set_tasks.
static int ad_check_tasks(const smaml_ctx* c, const char* who, int32_t nregions, const int32_t* tasks) {
  if (nregions <= 0 || !tasks) return fail(SMAML_EINVAL, std::string(who) + ": nregions must be positive and tasks_host set");
  const int nt = (int)c->feats.size();
  for (int r = 0; r < nregions; ++r) {
    if (tasks[r] < 0 || tasks[r] >= nt)
      return fail(SMAML_EINVAL, std::string(who) + ": region " + std::to_string(r) + ": task " + std::to_string(tasks[r]) +
                                    " out of range (" + std::to_string(nt) + " tasks set)");
    for (int q = 0; q < r; ++q)
      if (tasks[q] == tasks[r])
        return fail(SMAML_EINVAL, std::string(who) + ": duplicate task " + std::to_string(tasks[r]) + " (regions " +
                                      std::to_string(q) + " and " + std::to_string(r) + ")");
  }
  return SMAML_OK;
}

int smaml_adapt_prepare(smaml_ctx* c, void* stream, int32_t batch) {
  TRY(require_ready(c));
  TRY(check_lstm_dims(c->dims, "smaml_adapt_prepare"));
  if (c->feats.empty()) return fail(SMAML_ESTATE, "smaml_set_tasks not called");
  if (batch <= 0) return fail(SMAML_EINVAL, "bad adapt_prepare batch");
  TRY(ensure_device(c));
  bool cache = false;
  c->ad_ph = AdPhases{};
  const int32_t task0 = 0;
  return ad_prepare(c, (hipStream_t)stream, batch, &task0, 1, &cache);
}

// One call's adaptation steps: R regions (tasks of smaml_set_tasks) stepped in lockstep, every per-region array
// at the region's index -- theta / m / v [R][P], windows [nsteps][R][B], lr_dev and losses [nsteps][R], wd [R].
// gcn / gcn_m / gcn_v set: the GCN base trains too (one region; norms [nsteps] optional); null: a frozen base.
struct AdaptCall {
  const int32_t* tasks;
  int R;
  float *theta, *m, *v;
  float *gcn, *gcn_m, *gcn_v;
  int step0, nsteps, B;
  const int32_t* windows;
  const float* lr_dev;
  const float* wd;  // host
  float beta1, beta2, eps, max_norm;
  float* losses;
  float* norms;
  bool name_regions;  // window errors name the region, task and step (the lockstep entry point's wording)
};

// The buffers of a step that trains the base (af_buf): conv1..conv3's kept outputs, the GCN backward's two
// gradient buffers, k_gcn_dz's scratch, the step's windows side by side (B > 1) and the GCN gradient.
struct AfBufs {
  float* h[3];
  float *g, *gn, *top, *xcat, *ggrad;
};

// Every buffer of a base-training call before its first launch (a failure leaves the caller's vectors
// untouched); the feature cache (a frozen base's) is neither allocated nor read. From here on the base trains:
// gcn is the context's GCN parameter vector and cached features are stale.
static int af_prepare(smaml_ctx* c, hipStream_t s, const AdaptCall& a, int64_t nptr, AfBufs* f) {
  const Dims& d = c->d;
  const int B = a.B, rows = B * d.T * d.N;
  const int64_t hsz = (int64_t)rows * d.Hc, tsz = (int64_t)B * d.N * d.Hc, xsz = B > 1 ? (int64_t)rows * d.Cin0 : 0;
  const int64_t Pg = c->go.total;
  const bool fused_gcn = gcn_mlp_supported(d) && c->kn.gcn_fused;
  TRY(reserve(c, 1, B));
  if (c->af_buf.grow((5 * hsz + tsz + xsz + Pg) * 4) != hipSuccess ||
      c->bw_scratch.grow(2 * (int64_t)rows * std::max(d.Hc, d.Cin0) * 4) != hipSuccess ||
      (fused_gcn && c->gcn_wimg.grow(gcn_wimg_bytes(d)) != hipSuccess) ||
      c->xtab.grow(std::max<int64_t>(nptr, 1024) * (int64_t)sizeof(float*)) != hipSuccess)
    return fail(SMAML_ENOMEM, "smaml_adapt_steps_full: hipMalloc of the step's buffers failed (nothing was launched)");
  float* p = c->af_buf.as<float>();
  for (int l = 0; l < 3; ++l) f->h[l] = p + l * hsz;
  f->g = p + 3 * hsz;
  f->gn = f->g + hsz;
  f->top = f->gn + hsz;
  f->xcat = f->top + tsz;
  f->ggrad = f->xcat + xsz;
  // the gradient's pads are zeroed once per call: every step overwrites the tensors and leaves the pads
  HIP_TRY(hipMemsetAsync(f->ggrad, 0, (size_t)Pg * 4, s));
  c->gcn = a.gcn;
  ad_cache_invalidate(c);
  gc_invalidate(c);  // (the call trains the base in place)
  for (auto& x : c->af_stats) x = 0;
  return SMAML_OK;
}

// The adaptation step, once: nsteps steps of the call's regions, in launch sets of ad_group_size regions (Z = a
// set's regions on the task axis, per-task parameters at stride P; one region: stride 0). Per set and step:
// features -> LSTM -> head + loss -> backward (-> the GCN backward, base trained) -> clip + Adam. The features
// come from the cache slot itself (Z = 1), from the set's Z slots gathered into the workspace's F by one copy
// launch (k_gather_slabs, slot pointers uploaded with the window table), from the frozen forward (no cache: B > 1
// or GCN dropout), or from the keeping forward of a trained base. Cache fill: up front in batched GCN passes
// (adapt_gcn_batch > 1, or several regions); else the single region's window on its first use, counted in
// ad_ph.filled.
static int adapt_run(smaml_ctx* c, hipStream_t s, const AdaptCall& a) {
  using clk = std::chrono::steady_clock;
  const Dims& d = c->d;
  const int B = a.B, R = a.R, nsteps = a.nsteps;
  const bool train = a.gcn != nullptr;
  if (train && R != 1) return fail(SMAML_EINVAL, "internal: adapt_run trains the base of one region only");
  TRY(check_loss_weights(c, a.name_regions ? "smaml_adapt_steps_multi" : "smaml_adapt_steps"));
  // one table for the call: the window pointers [nsteps][R][B], then (cache) the slot pointers [nsteps][R]
  const int64_t nwin = (int64_t)nsteps * R * B, nslot = (int64_t)nsteps * R;
  std::vector<const float*> ptrs(nwin);
  for (int64_t i = 0; i < nwin; ++i) {
    const int r = (int)(i / B % R), task = a.tasks[r];
    const int wv = a.windows[i];
    if (wv < 0 || wv + d.T + d.Hf >= c->t_total[task]) {
      if (!a.name_regions) return fail(SMAML_EINVAL, "window start out of range");
      return fail(SMAML_EINVAL, "adapt_steps_multi: region " + std::to_string(r) + " (task " + std::to_string(task) +
                                    "): window " + std::to_string(wv) + " of step " + std::to_string(i / B / R) +
                                    " out of range (stream of " + std::to_string(c->t_total[task]) + " rows)");
    }
    ptrs[i] = c->feats[task] + (int64_t)wv * d.N * d.Cin0;
  }
  if (train && (int64_t)B * d.T * d.N * std::max(d.Hc, 4 * d.H) >= (1ll << 31))
    return fail(SMAML_EINVAL, "batch too large: B*T*N*max(Hc, 4H) must stay below 2^31");
  TRY(ensure_device(c));
  c->ad_ph = AdPhases{};
  bool cache = false;
  AfBufs f{};
  if (train) {
    TRY(check_device_error(c));
    TRY(af_prepare(c, s, a, nwin, &f));
  } else {
    TRY(ad_prepare(c, s, B, a.tasks, R, &cache));  // no allocation after smaml_adapt_prepare[_multi] / an earlier call
  }
  const int G = ad_group_size(c, R);  // regions per launch set
  const int64_t P = c->po.P, Pg = c->go.total;
  const int64_t fsz = (int64_t)d.T * d.N * d.Hc;  // floats of one window's features
  const int rows = B * d.T * d.N;
  const float inv = 1.f / ((float)d.N * d.HfC * B);
  const bool dropout = c->p_gcn > 0.f || c->p_lstm > 0.f;
  if (dropout) {  // masks keyed by each region's task id (smaml_set_task_ids; default: the task index)
    std::vector<int32_t> ids(R);
    for (int r = 0; r < R; ++r) ids[r] = a.tasks[r] < (int)c->task_ids.size() ? c->task_ids[a.tasks[r]] : a.tasks[r];
    TRY(c->stage.upload(s, c->task_id_dev, ids.data(), (int64_t)R * 4));
  }
  if (c->lw_sets > 1) {  // region r reads the set of its task index (a single region: task 0, set 0)
    HIP_TRY(c->lw_zset.grow((int64_t)R * 4));
    TRY(c->stage.upload(s, c->lw_zset.ptr, a.tasks, (int64_t)R * 4));
  }
  // Batch-1 steps without GCN dropout reuse each window's GCN features across epochs (F2; cache implies B = 1).
  auto t0 = clk::now();
  if (cache) {
    if (c->ad_gcn_batch > 1 || R > 1) {  // every region's missing windows up front, region by region
      for (int r = 0; r < R; ++r) TRY(ad_cache_fill(c, s, a.tasks[r], a.windows + r, nsteps, R));
      if (c->ad_phase_sync) HIP_TRY(hipStreamSynchronize(s));
    }
    ptrs.resize(nwin + nslot);
    for (int64_t i = 0; i < nslot; ++i)
      ptrs[nwin + i] = c->ad[a.tasks[i % R]].F.as<float>() + (int64_t)a.windows[i] * fsz;
  }
  auto t1 = clk::now();
  TRY(upload_xtab(c, s, ptrs.data(), (int64_t)ptrs.size()));
  for (int k = 0; k < nsteps; ++k) {
    for (int r0 = 0; r0 < R; r0 += G) {
      const int Z = std::min(G, R - r0);
      set_work(c, Z, B);  // (ends a pending smaml_forward / smaml_backward pair)
      use_loss_weights(c, c->lw_sets > 1 ? c->lw_zset.as<int32_t>() + r0 : nullptr);
      Work& w = c->w;
      // (one region: the parameters at stride 0)
      float* th = a.theta + (int64_t)r0 * P;
      const int64_t ts = Z > 1 ? P : 0;
      const int64_t at = (int64_t)k * R + r0;  // the set's first region in the per-step arrays
      const float* const* xt = nullptr;
      TRY(xtab_at(c, at * B, &xt));
      if (dropout) {
        set_step_drop(c, a.step0 + k);
        w.drop.task_id = c->task_id_dev + r0;
      }
      if (train) {
        if (c->gcn_keep) {
          TRY(run_gcn_keep(c, s, xt, f.h, c->af_stats));
        } else {  // A/B: the frozen-base forward, then conv1..conv3 recomputed on the per-layer path (smaml_backward_base)
          TRY(run_gcn(c, s, xt));
          for (int l = 0; l < 3; ++l) {
            TIMED(c, s, C_GCN, 2.0 * rows * c->go.cin[l] * d.Hc,
                  launch_gcn_layer(s, d, l, B, B, l == 0 ? xt : nullptr, l == 0 ? nullptr : f.h[l - 1], f.h[l], false, true,
                                   c->gcn + c->go.w[l], c->gcn + c->go.b[l], c->go.cin[l], d.Hc, graph_view(c), d.T * d.N, d.N, &w.drop));
            c->af_stats[5] += 1;
          }
        }
        TRY(run_lstm(c, s, th, ts));
      } else if (cache) {
        if (Z == 1) {
          const int task = a.tasks[r0], wv = a.windows[at];
          w.F = const_cast<float*>(ptrs[nwin + at]);  // the slot itself
          if (!c->ad[task].valid[wv]) {
            TRY(run_gcn(c, s, xt));  // writes the window's features straight into its cache slot
            c->ad[task].valid[wv] = 1;
            c->ad_ph.filled += 1;
          }
        } else {
          const float* const* st = nullptr;
          TRY(xtab_at(c, nwin + at, &st));
          TIMED(c, s, C_GCN, 0, launch_gather_slabs(s, st, Z, fsz, c->F_main));
        }
        TRY(run_lstm(c, s, th, ts));
      } else {
        TRY(run_forward(c, s, th, ts, xt));
      }
      TIMED(c, s, C_HEAD, 2.0 * Z * w.M * d.HfC * d.H, launch_head_loss(s, d, w, th, ts, c->po, xt, 2.f * inv, true));
      TRY(run_backward(c, s, th, ts, c->grad));
      if (train) {
        // dZ4 = dF through conv4's ReLU, per sample: layer 0's dG slab (left by the BPTT) times W_ih0
        TIMED(c, s, C_MISC, 2.0 * rows * 4 * d.H * d.Hc,
              launch_lstm_dx0(s, d, w, w.dG, th + c->po.lay[0].wih, w.F, f.g));
        const float* x0 = ptrs[at * B];  // B = 1: the window is [T*N][Cin0] in the stream already
        if (B > 1) {
          const int64_t xsz = (int64_t)d.T * d.N * d.Cin0;
          for (int si = 0; si < B; ++si)
            HIP_TRY(hipMemcpyAsync(f.xcat + si * xsz, ptrs[at * B + si], (size_t)xsz * 4, hipMemcpyDeviceToDevice, s));
          x0 = f.xcat;
        }
        // (conv1's input gradient: nothing reads it)
        TRY(gcn_backward_chain(c, s, x0, f.h, f.g, f.gn, rows, d.T * d.N, a.gcn, f.ggrad, false,
                               c->gcn_dz_fused ? f.top : nullptr, c->af_stats, C_MISC));
        c->af_stats[0] += 1;
      }
      // (the step's loss is summed by the Adam launch's first block: the backward leaves the head's partials alone)
      AdamL2 u{};
      u.seg[0] = {th, c->grad, a.m + (int64_t)r0 * P, a.v + (int64_t)r0 * P, P};
      u.seg[1] = {a.gcn, f.ggrad, a.gcn_m, a.gcn_v, Pg};
      u.S = train ? 2 : 1;
      u.R = Z;
      u.part = w.sqpart;
      u.lr_dev = a.lr_dev + at;
      for (int z = 0; z < Z; ++z) u.wd.wd[z] = a.wd[r0 + z];
      u.step = a.step0 + k + 1;
      u.b1 = a.beta1, u.b2 = a.beta2, u.eps = a.eps, u.max_norm = a.max_norm;
      u.lpart = w.lpart, u.lblocks = w.lblocks, u.inv_count = inv;
      u.loss = a.losses + at;
      u.norm_out = a.norms ? a.norms + at : nullptr;
      TIMED(c, s, C_MISC, 0, launch_adam_l2(s, u));
    }
  }
  if (c->ad_phase_sync) HIP_TRY(hipStreamSynchronize(s));
  auto t2 = clk::now();
  c->ad_ph.ms[AD_FILL] = std::chrono::duration<double, std::milli>(t1 - t0).count();
  c->ad_ph.ms[AD_STEPS] = std::chrono::duration<double, std::milli>(t2 - t1).count();
  c->w.F = c->F_main;
  c->w.drop = Drop{};
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_adapt_steps(smaml_ctx* c, void* stream, float* theta, float* m, float* v, int32_t step0, int32_t nsteps,
                      int32_t batch, const int32_t* windows_host, const float* lr_dev, float beta1, float beta2,
                      float eps, float weight_decay, float max_norm, float* losses) {
  TRY(require_ready(c));
  TRY(check_lstm_dims(c->dims, "smaml_adapt_steps"));
  if (c->feats.empty()) return fail(SMAML_ESTATE, "smaml_set_tasks not called");
  if (!theta || !m || !v || nsteps <= 0 || batch <= 0 || !windows_host || !lr_dev || !losses || step0 < 0)
    return fail(SMAML_EINVAL, "bad adapt_steps arguments");
  const int32_t task0 = 0;
  return adapt_run(c, (hipStream_t)stream,
                   AdaptCall{&task0, 1, theta, m, v, nullptr, nullptr, nullptr, step0, nsteps, batch, windows_host, lr_dev,
                             &weight_decay, beta1, beta2, eps, max_norm, losses, nullptr, false});
}

int smaml_adapt_steps_full(smaml_ctx* c, void* stream, float* theta, float* m, float* v, float* gcn, float* gcn_m,
                           float* gcn_v, int32_t step0, int32_t nsteps, int32_t batch, const int32_t* windows_host,
                           const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                           float max_norm, float* losses, float* norms) {
  // (the checks that need no context first: they run without a device too)
  if (!theta || !m || !v || !gcn || !gcn_m || !gcn_v || !windows_host || !lr_dev || !losses)
    return fail(SMAML_EINVAL, "smaml_adapt_steps_full: NULL argument");
  if (nsteps <= 0 || batch <= 0 || step0 < 0)
    return fail(SMAML_EINVAL, "smaml_adapt_steps_full: nsteps and batch must be positive, step0 non-negative");
  if (!aligned16(theta) || !aligned16(m) || !aligned16(v) || !aligned16(gcn) || !aligned16(gcn_m) || !aligned16(gcn_v))
    return fail(SMAML_EINVAL, "smaml_adapt_steps_full: theta, m, v, gcn, gcn_m, gcn_v must be 16-byte aligned");
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  if (!graph_set(c)) return fail(SMAML_ESTATE, "smaml_set_graph not called");
  TRY(check_lstm_dims(c->dims, "smaml_adapt_steps_full"));
  if (c->feats.empty()) return fail(SMAML_ESTATE, "smaml_set_tasks not called");
  const int32_t task0 = 0;
  return adapt_run(c, (hipStream_t)stream,
                   AdaptCall{&task0, 1, theta, m, v, gcn, gcn_m, gcn_v, step0, nsteps, batch, windows_host, lr_dev,
                             &weight_decay, beta1, beta2, eps, max_norm, losses, norms, false});
}

int smaml_adapt_full_stats(const smaml_ctx* c, int64_t* counts, int32_t cap, int32_t* count) {
  if (!c || cap < 0 || (cap > 0 && !counts)) return fail(SMAML_EINVAL, "bad adapt_full_stats arguments");
  for (int i = 0; i < 6 && i < cap; ++i) counts[i] = c->af_stats[i];
  if (count) *count = 6;
  return SMAML_OK;
}

int smaml_adapt_prepare_multi(smaml_ctx* c, void* stream, int32_t nregions, const int32_t* tasks_host, int32_t batch) {
  TRY(require_ready(c));
  TRY(check_lstm_dims(c->dims, "smaml_adapt_prepare_multi"));
  if (c->feats.empty()) return fail(SMAML_ESTATE, "smaml_set_tasks not called");
  if (batch <= 0) return fail(SMAML_EINVAL, "bad adapt_prepare_multi batch");
  TRY(ad_check_tasks(c, "adapt_prepare_multi", nregions, tasks_host));
  TRY(ensure_device(c));
  bool cache = false;
  c->ad_ph = AdPhases{};
  return ad_prepare(c, (hipStream_t)stream, batch, tasks_host, nregions, &cache);
}

// R regions' fine-tuning in lockstep (adapt_run): step k of every region of a launch set as ONE set of launches
// over the task axis, as the MAML inner loop runs its tasks. The regions of a set are consecutive entries of
// tasks_host, so their theta / m / v / lr / loss slabs are the caller's arrays at the set's offset.
int smaml_adapt_steps_multi(smaml_ctx* c, void* stream, int32_t nregions, const int32_t* tasks_host, float* theta,
                            float* m, float* v, int32_t step0, int32_t nsteps, int32_t batch,
                            const int32_t* windows_host, const float* lr_dev, const float* weight_decay_host,
                            float beta1, float beta2, float eps, float max_norm, float* losses) {
  TRY(require_ready(c));
  TRY(check_lstm_dims(c->dims, "smaml_adapt_steps_multi"));
  if (c->feats.empty()) return fail(SMAML_ESTATE, "smaml_set_tasks not called");
  if (!theta || !m || !v || nsteps <= 0 || batch <= 0 || !windows_host || !lr_dev || !weight_decay_host || !losses ||
      step0 < 0)
    return fail(SMAML_EINVAL, "bad adapt_steps_multi arguments");
  TRY(ad_check_tasks(c, "adapt_steps_multi", nregions, tasks_host));
  return adapt_run(c, (hipStream_t)stream,
                   AdaptCall{tasks_host, nregions, theta, m, v, nullptr, nullptr, nullptr, step0, nsteps, batch,
                             windows_host, lr_dev, weight_decay_host, beta1, beta2, eps, max_norm, losses, nullptr, true});
}

int smaml_adapt_phases(const smaml_ctx* c, double* ms, int32_t cap, int32_t* count, int64_t* filled) {
  if (!c || cap < 0 || (cap > 0 && !ms)) return fail(SMAML_EINVAL, "bad adapt_phases arguments");
  for (int i = 0; i < AD_NPH && i < cap; ++i) ms[i] = c->ad_ph.ms[i];
  if (count) *count = AD_NPH;
  if (filled) *filled = c->ad_ph.filled;
  return SMAML_OK;
}

int smaml_timing(smaml_ctx* c, int32_t enable) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  c->tm.on = enable != 0;
  return SMAML_OK;
}

int smaml_timing_collect(smaml_ctx* c, double* ms, double* flops, int64_t* count, int32_t cap) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  TRY(ensure_device(c));
  HIP_TRY(hipDeviceSynchronize());
  for (auto& r : c->tm.recs) {
    float e = 0.f;
    HIP_TRY(hipEventElapsedTime(&e, r.a, r.b));
    c->tm.ms[r.cat] += e;
    c->tm.flops[r.cat] += r.flops;
    c->tm.count[r.cat] += 1;
    c->tm.pool.push_back(r.a);
    c->tm.pool.push_back(r.b);
  }
  c->tm.recs.clear();
  for (int i = 0; i < NCAT && i < cap; ++i) {
    if (ms) ms[i] = c->tm.ms[i];
    if (flops) flops[i] = c->tm.flops[i];
    if (count) count[i] = c->tm.count[i];
    c->tm.ms[i] = 0;
    c->tm.flops[i] = 0;
    c->tm.count[i] = 0;
  }
  return SMAML_OK;
}

int smaml_variant_counts(smaml_ctx* c, int64_t* counts, int32_t cap, int32_t* count, int32_t reset) {
  if (!c || cap < 0 || (cap > 0 && !counts)) return fail(SMAML_EINVAL, "bad variant_counts arguments");
  for (int i = 0; i < NVAR && i < cap; ++i) counts[i] = c->vcount[i];
  if (count) *count = NVAR;
  if (reset)
    for (auto& v : c->vcount) v = 0;
  return SMAML_OK;
}

int smaml_set_option(smaml_ctx* c, const char* key, int64_t value) {
  if (!c || !key) return fail(SMAML_EINVAL, "NULL argument");
  const std::string k(key);
  if (k == "bwd_big_min" && value >= 0) {
    c->kn.bwd_big_min = (int)std::min<int64_t>(value, 1 << 30);
  } else if (k == "bwdd_big_min" && value >= 0) {
    c->kn.bwdd_big_min = (int)std::min<int64_t>(value, 1 << 30);
  } else if (k == "split_max" && value >= 1) {
    c->kn.split_max = (int)std::min<int64_t>(value, 64);
  } else if (k == "wgrad_group_max_rows" && value >= 0) {
    c->kn.wgrad_group_max_rows = (int)std::min<int64_t>(value, 1 << 30);
  } else if (k == "gcn_fused" && (value == 0 || value == 1)) {
    c->kn.gcn_fused = (int)value;
  } else if (k == "gate_img" && (value == 0 || value == 1)) {
    c->kn.gate_img = (int)value;
  } else if (k == "wgrad_wide" && (value == 0 || value == 1)) {
    c->kn.wgrad_wide = (int)value;
  } else if (k == "wgrad_pair" && (value == 0 || value == 1)) {
    c->kn.wgrad_pair = (int)value;
  } else if (k == "bwdd_remap" && (value == 0 || value == 1)) {
    c->kn.bwdd_remap = (int)value;
  } else if (k == "small_kw" && value >= 0 && value <= 2) {
    c->kn.small_kw = (int)value;
  } else if (k == "gcn_dedup" && (value == 0 || value == 1)) {
    c->kn.gcn_dedup = (int)value;
  } else if (k == "so_f_store" && (value == 0 || value == 1)) {
    c->so_f_store = (int)value;
  } else if (k == "gcn_stream_cache" && (value == 0 || value == 1)) {
    c->gc_on = (int)value;
  } else if (k == "gcn_stream_cache_mb" && value >= -1 && value <= (1 << 24)) {
    c->gc_budget_mb = value;
    if (value >= 0) gc_drop(c);  // (re-planned under the new cap by the next meta-step)
  } else if (k == "xg_dedup" && (value == 0 || value == 1)) {
    c->kn.xg_dedup = (int)value;
  } else if (k == "wgrad_dedup" && (value == 0 || value == 1)) {
    c->kn.wgrad_dedup = (int)value;
  } else if (k == "bptt_streams" && value >= 1 && value <= 4) {
    c->kn.bptt_streams = (int)value;
  } else if (k == "f_compact" && (value == 0 || value == 1)) {
    c->kn.f_compact = (int)value;
  } else if (k == "fwd_streams" && value >= 0 && value <= 4) {
    c->kn.fwd_streams = (int)value;
  } else if (k == "adapt_phase_sync" && (value == 0 || value == 1)) {
    c->ad_phase_sync = (int)value;
  } else if (k == "adapt_group" && value >= -1 && value <= ADAPT_MAX_GROUP) {
    c->ad_group = (int)value;
  } else if (k == "roll_reuse" && (value == 0 || value == 1)) {
    c->roll_reuse = (int)value;
  } else if (k == "ens_share" && (value == 0 || value == 1)) {
    c->ens_share = (int)value;
  } else if (k == "ens_group" && value >= -1 && value <= 64) {
    c->ens_group = (int)value;
  } else if (k == "roll_ens_budget_mb" && value >= 1 && value <= (1 << 20)) {
    c->roll_ens_budget_mb = value;
  } else if (k == "dx0_fused" && (value == 0 || value == 1)) {
    c->dx0_fused = (int)value;
  } else if (k == "gcn_keep" && (value == 0 || value == 1)) {
    c->gcn_keep = (int)value;
  } else if (k == "gcn_dz_fused" && (value == 0 || value == 1)) {
    c->gcn_dz_fused = (int)value;
  } else if (k == "meta_base_dedup" && (value == 0 || value == 1)) {
    c->meta_base_dedup = (int)value;
  } else if (k == "adapt_gcn_batch" && value >= 0 && value <= 256) {
    c->ad_gcn_batch = (int)value;
  } else if (k == "wgrad_group_wgs" && value >= 1) {
    c->kn.wgrad_group_wgs = (int)std::min<int64_t>(value, 1 << 20);
  } else if (k == "grid_barrier" && (value == 0 || value == 1)) {
    c->bar_fused = (int)value;
  } else if (k == "barrier_timeout_us" && value >= 1) {
    c->bar_timeout_us = std::min<int64_t>(value, 600000000);
  } else if (k == "comm_timeout_ms" && value >= 1) {
    c->comm_timeout_ms = std::min<int64_t>(value, 3600000);
  } else if (k == "barrier_oversize" && value >= 0 && value <= 64) {
    c->bar_oversize = (int)value;
  } else if (k == "keep" && value >= -1) {
    c->keep_max = (int)std::min<int64_t>(value, 1 << 20);
    c->keep_tried_K = -1;  // re-plan the kept slots on the next second-order meta-step
  } else {
    return fail(SMAML_EINVAL, "unknown option or bad value: " + k);
  }
  return SMAML_OK;
}

int smaml_adamw_step(smaml_ctx* c, void* stream, float* theta, const float* grad, float* m, float* v, int64_t n,
                     int32_t step, float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                     float* norm_out) {
  if (!c || !theta || !grad || !m || !v || n <= 0 || step < 1) return fail(SMAML_EINVAL, "bad adamw arguments");
  TRY(ensure_device(c));
  TRY(check_device_error(c));
  TRY(reserve(c, 1, 1));
  hipStream_t s = (hipStream_t)stream;
  const double bc1 = 1.0 - std::pow((double)beta1, step);
  const double bc2 = 1.0 - std::pow((double)beta2, step);
  launch_adamw(s, theta, grad, m, v, n, c->w.sqpart + (int64_t)c->z_cap * SQB, lr, beta1, beta2, eps, weight_decay,
               (float)(lr / bc1), (float)std::sqrt(bc2), max_norm, norm_out);
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

// ---- finer-grained entry points --------------------------------------

int smaml_backward(smaml_ctx* c, void* stream, const float* theta, const float* dpred, float* grad) {
  TRY(require_ready(c));
  TRY(check_lstm_dims(c->dims, "smaml_backward"));
  if (!theta || !dpred || !grad) return fail(SMAML_EINVAL, "bad backward arguments");
  if (c->act_B < 1 || c->w.Z != 1) return fail(SMAML_ESTATE, "smaml_backward needs the activations of smaml_forward");
  TRY(ensure_device(c));
  hipStream_t s = (hipStream_t)stream;
  const Dims& d = c->d;
  // dpred [B][N*Hf][C] (rows n*Hf+h) == w.dpred [M = B*N][Hf*C]: same flat order
  HIP_TRY(hipMemcpyAsync(c->w.dpred, dpred, (size_t)c->w.M * d.HfC * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemsetAsync(grad, 0, (size_t)c->po.P * 4, s));
  c->act_B = -1;  // the BPTT overwrites the saved gates with dG
  TRY(run_backward(c, s, theta, 0, grad));
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_backward_base(smaml_ctx* c, void* stream, const float* theta, const float* const* x_host, int32_t nsamples,
                        const float* dpred, float* grad, float* gcn_grad, float* const* dx_host) {
  // (the checks that need no context first: they run without a device too)
  if (!gcn_grad && !dx_host)
    return fail(SMAML_EINVAL, "smaml_backward_base: gcn_grad and dx_host are both NULL (use smaml_backward)");
  if (!theta || !x_host || nsamples <= 0 || !dpred || !grad)
    return fail(SMAML_EINVAL, "bad backward_base arguments");
  TRY(require_ready(c));
  TRY(check_lstm_dims(c->dims, "smaml_backward_base"));
  if (c->act_B < 1 || c->w.Z != 1)
    return fail(SMAML_ESTATE, "smaml_backward_base needs the activations of smaml_forward");
  if (nsamples != c->act_B)
    return fail(SMAML_ESTATE, "smaml_backward_base: " + std::to_string(nsamples) + " samples, but the forward ran " +
                                  std::to_string(c->act_B));
  if (c->w.fcompact) return fail(SMAML_ESTATE, "internal: smaml_forward left compact features");
  for (int i = 0; i < nsamples; ++i) {
    if (!x_host[i] || !aligned16(x_host[i])) return fail(SMAML_EINVAL, "sample x pointers must be 16-B aligned");
    if (dx_host && (!dx_host[i] || !aligned16(dx_host[i])))
      return fail(SMAML_EINVAL, "sample dx pointers must be 16-B aligned");
  }
  if (gcn_grad && !aligned16(gcn_grad)) return fail(SMAML_EINVAL, "gcn_grad must be 16-byte aligned");
  TRY(ensure_device(c));
  hipStream_t s = (hipStream_t)stream;
  const Dims& d = c->d;
  Work& w = c->w;
  const int rps = d.T * d.N, R = nsamples * rps;
  const int Wd = std::max(d.Hc, d.Cin0);
  const int64_t hsz = (int64_t)R * d.Hc, gsz = (int64_t)R * Wd, xsz = (int64_t)R * d.Cin0;
  // every buffer before the first launch (a grow releases the old buffer after a device sync)
  if (c->bg_buf.grow((3 * hsz + 2 * gsz + xsz) * 4) != hipSuccess || c->bw_scratch.grow(2 * gsz * 4) != hipSuccess)
    return fail(SMAML_ENOMEM, "smaml_backward_base: hipMalloc of the GCN backward's buffers failed (the forward's "
                              "activations are still valid)");
  float* h[3] = {c->bg_buf.as<float>(), c->bg_buf.as<float>() + hsz, c->bg_buf.as<float>() + 2 * hsz};
  float* g = h[2] + hsz;
  float* gn = g + gsz;
  float* xcat = gn + gsz;
  // smaml_backward's part: the same launches in the same order
  HIP_TRY(hipMemcpyAsync(w.dpred, dpred, (size_t)w.M * d.HfC * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemsetAsync(grad, 0, (size_t)c->po.P * 4, s));
  c->act_B = -1;  // the BPTT overwrites the saved gates with dG
  TRY(run_backward(c, s, theta, 0, grad));
  // conv1..conv3's outputs (post-ReLU, post-dropout) on the per-layer path with the forward's masks (w.drop):
  // the forward's fused GCN kept them in registers
  TRY(upload_xtab(c, s, x_host, nsamples));
  const float* const* xt = nullptr;
  TRY(xtab_at(c, 0, &xt));
  const GraphView gv = graph_view(c);
  for (int k = 0; k < 3; ++k)
    TIMED(c, s, C_GCN, 2.0 * R * c->go.cin[k] * d.Hc,
          launch_gcn_layer(s, d, k, nsamples, nsamples, k == 0 ? xt : nullptr, k == 0 ? nullptr : h[k - 1], h[k], false,
                           true, c->gcn + c->go.w[k], c->gcn + c->go.b[k], c->go.cin[k], d.Hc, gv, rps, d.N,
                           &w.drop));
  // dZ4 = dF through conv4's ReLU, per sample: layer 0's dG slab (left by the BPTT) times W_ih0
  const float* Wih0 = theta + c->po.lay[0].wih;
  const double fl0 = 2.0 * R * 4 * d.H * d.Hc;
  if (c->dx0_fused) {
    TIMED(c, s, C_MISC, fl0, launch_lstm_dx0(s, d, w, w.dG, Wih0, w.F, g));
  } else {  // the composed form it replaces (A/B): GEMM, ReLU mask, T strided copies per sample
    const int64_t blk = (int64_t)d.N * d.Hc;
    TIMED(c, s, C_MISC, fl0, {
      launch_gemm_nn_plain(s, w.dG, d.T * w.M, 4 * d.H, Wih0, d.Hc, gn);
      launch_relu_mask(s, gn, w.F, hsz);
      for (int si = 0; si < nsamples; ++si)  // [T][M][Hc] -> [s][T*N][Hc]
        (void)hipMemcpy2DAsync(g + (int64_t)si * d.T * blk, blk * 4, gn + (int64_t)si * blk, (int64_t)nsamples * blk * 4,
                               blk * 4, d.T, hipMemcpyDeviceToDevice, s);
    });
  }
  if (gcn_grad) {
    HIP_TRY(hipMemsetAsync(gcn_grad, 0, (size_t)c->go.total * 4, s));  // the pads stay zero
    for (int si = 0; si < nsamples; ++si)
      HIP_TRY(hipMemcpyAsync(xcat + (int64_t)si * rps * d.Cin0, x_host[si], (size_t)rps * d.Cin0 * 4,
                             hipMemcpyDeviceToDevice, s));
  }
  // conv4 -> conv1 (conv4's ReLU is in dZ4 already), the three-launch form of the layer-to-layer gradient; timed
  // with the recompute above (C_GCN), so that C_MISC stays the layer-0 input gradient alone (tools/bench_base_grad.py)
  TRY(gcn_backward_chain(c, s, xcat, h, g, gn, R, rps, c->gcn, gcn_grad, dx_host != nullptr, nullptr, nullptr, C_GCN));
  if (dx_host)
    for (int si = 0; si < nsamples; ++si)
      HIP_TRY(hipMemcpyAsync(dx_host[si], g + (int64_t)si * rps * d.Cin0, (size_t)rps * d.Cin0 * 4,
                             hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_dropout(smaml_ctx* c, void* stream, float* x, int64_t n, float p, uint32_t seed, int32_t layer) {
  if (!c || !x || n < 0 || !(p >= 0.f && p < 1.f) || layer < 0) return fail(SMAML_EINVAL, "bad dropout arguments");
  TRY(ensure_device(c));
  if (p > 0.f && n > 0) launch_dropout_inplace((hipStream_t)stream, x, n, p, seed, layer);
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_gcn_forward(smaml_ctx* c, void* stream, const float* const* x_host, int32_t nsamples, float* feats) {
  TRY(require_ready(c));
  if (!x_host || nsamples <= 0 || !feats) return fail(SMAML_EINVAL, "bad gcn_forward arguments");
  for (int i = 0; i < nsamples; ++i)
    if (!x_host[i] || !aligned16(x_host[i])) return fail(SMAML_EINVAL, "sample x pointers must be 16-B aligned");
  TRY(ensure_device(c));
  hipStream_t s = (hipStream_t)stream;
  TRY(reserve(c, 1, nsamples));
  set_work(c, 1, nsamples);
  TRY(upload_xtab(c, s, x_host, nsamples));
  const float* const* xt = nullptr;
  TRY(xtab_at(c, 0, &xt));
  TRY(run_gcn(c, s, xt));
  const Dims& d = c->d;
  const int64_t blk = (int64_t)d.N * d.Hc;
  for (int si = 0; si < nsamples; ++si)  // F [T][M][Hc] -> feats [s][T*N][Hc]
    HIP_TRY(hipMemcpy2DAsync(feats + (int64_t)si * d.T * blk, blk * 4, c->w.F + (int64_t)si * blk,
                             (int64_t)nsamples * blk * 4, blk * 4, d.T, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_lstm_forward(smaml_ctx* c, void* stream, const float* theta, const float* feats, int32_t nsamples,
                       float* hT) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  TRY(check_lstm_dims(c->dims, "smaml_lstm_forward"));
  if (!theta || !feats || nsamples <= 0 || !hT) return fail(SMAML_EINVAL, "bad lstm_forward arguments");
  TRY(ensure_device(c));
  hipStream_t s = (hipStream_t)stream;
  TRY(reserve(c, 1, nsamples));
  set_work(c, 1, nsamples);
  const Dims& d = c->d;
  const int64_t blk = (int64_t)d.N * d.Hc;
  for (int si = 0; si < nsamples; ++si)  // feats [s][T*N][Hc] -> F [T][M][Hc]
    HIP_TRY(hipMemcpy2DAsync(c->w.F + (int64_t)si * blk, (int64_t)nsamples * blk * 4, feats + (int64_t)si * d.T * blk,
                             blk * 4, blk * 4, d.T, hipMemcpyDeviceToDevice, s));
  TRY(run_lstm(c, s, theta, 0));
  const int64_t lsz = (int64_t)d.T * c->w.M * d.H;
  const float* top = c->w.Hs + (int64_t)(d.L - 1) * lsz + (int64_t)(d.T - 1) * c->w.M * d.H;
  HIP_TRY(hipMemcpyAsync(hT, top, (size_t)c->w.M * d.H * 4, hipMemcpyDeviceToDevice, s));
  c->act_B = nsamples;
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_lstm_backward(smaml_ctx* c, void* stream, const float* theta, const float* dhT, float* grad) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  TRY(check_lstm_dims(c->dims, "smaml_lstm_backward"));
  if (!theta || !dhT || !grad) return fail(SMAML_EINVAL, "bad lstm_backward arguments");
  if (c->act_B < 1 || c->w.Z != 1)
    return fail(SMAML_ESTATE, "smaml_lstm_backward needs the activations of smaml_lstm_forward");
  TRY(ensure_device(c));
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(c->w.dH, dhT, (size_t)c->w.M * c->d.H * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemsetAsync(grad, 0, (size_t)c->po.P * 4, s));
  c->act_B = -1;
  TRY(run_bptt(c, s, theta, 0, grad));
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_head_loss(smaml_ctx* c, void* stream, const float* theta, const float* hT, const float* const* y_host,
                    int32_t nsamples, float* pred, float* loss, float* dpred) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  TRY(check_lstm_dims(c->dims, "smaml_head_loss"));
  if (!theta || !hT || nsamples <= 0 || !pred) return fail(SMAML_EINVAL, "bad head_loss arguments");
  if (y_host && (!loss || !dpred)) return fail(SMAML_EINVAL, "loss and dpred are required with targets");
  if (!aligned16(hT) || !aligned16(theta)) return fail(SMAML_EINVAL, "hT / theta must be 16-byte aligned");
  TRY(ensure_device(c));
  hipStream_t s = (hipStream_t)stream;
  // the head only needs the small per-launch buffers; keep saved LSTM activations intact
  if (nsamples > c->zb_cap) TRY(reserve(c, 1, nsamples));
  const int act = c->act_B;
  const Work saved = c->w;
  set_work(c, 1, nsamples);
  if (c->lw_sets > 0) {  // set 0, whatever the number of sets
    use_loss_weights(c, nullptr);
    c->w.lw.zstride = 0;
    c->w.lw.zset = nullptr;
  }
  if (y_host) {
    for (int i = 0; i < nsamples; ++i)
      if (!y_host[i]) return fail(SMAML_EINVAL, "null target pointer");
    TRY(upload_xtab(c, s, y_host, nsamples));
  }
  const float* const* yt = nullptr;
  if (y_host) TRY(xtab_at(c, 0, &yt));
  const Dims& d = c->d;
  const float inv = 1.f / ((float)nsamples * d.N * d.HfC);  // mean over samples and elements (F9)
  launch_head_loss_y(s, d, c->w, hT, theta, c->po, yt, pred, dpred, 2.f * inv);
  if (y_host) launch_loss_final(s, c->w, inv, loss);
  c->w = saved;
  c->act_B = act;
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_clip_sgd(smaml_ctx* c, void* stream, float* theta, const float* grad, int32_t ntasks, float lr,
                   float max_norm, float* norms) {
  if (!c || !theta || !grad || ntasks <= 0) return fail(SMAML_EINVAL, "bad clip_sgd arguments");
  TRY(ensure_device(c));
  if (ntasks > c->z_cap) TRY(reserve(c, ntasks, 1));
  TRY(ensure_bar(c));
  hipStream_t s = (hipStream_t)stream;
  TRY(check_device_error(c));
  HIP_TRY(launch_inner_sgd(s, theta, grad, c->po.P, ntasks, c->w.sqpart, lr, max_norm, norms, nullptr, bar_plan(c)));
  HIP_TRY(hipGetLastError());
  return SMAML_OK;
}

int smaml_sync(smaml_ctx* c, void* stream) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  TRY(ensure_device(c));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return check_device_error(c);
}

int smaml_inner_loop(smaml_ctx* c, void* stream, const float* theta, int32_t steps, int32_t batch,
                     const int32_t* windows_host, float inner_lr, float max_norm, float* fast_out, float* losses,
                     float* norms) {
  if (!fast_out) return fail(SMAML_EINVAL, "fast_out is required");
  return smaml_meta_step(c, stream, theta, 0, steps, batch, windows_host, inner_lr, max_norm, 1.f, nullptr, losses,
                         norms, fast_out);
}

int smaml_alloc(smaml_ctx* c, int64_t bytes, void** out) {
  if (!c || bytes <= 0 || !out) return fail(SMAML_EINVAL, "bad alloc arguments");
  TRY(ensure_device(c));
  if (hipMalloc(out, (size_t)bytes) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return fail(SMAML_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " B failed");
  }
  return SMAML_OK;
}

int smaml_free(smaml_ctx* c, void* p) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  if (!p) return SMAML_OK;
  TRY(ensure_device(c));
  HIP_TRY(hipFree(p));
  return SMAML_OK;
}

}  // extern "C"

// ---- RCCL communicator (one process per GPU). librccl is resolved at first use with dlopen,
// so the library has no link-time RCCL dependency (and shares the process's RCCL if torch
// has already loaded one). Only the handful of symbols below are used.
namespace {
// ncclConfig_t as of NCCL 2.14 (size / magic / version + the first user fields): the library reads only
// the fields the declared version has, so this prefix works with the RCCL torch bundles and /opt/rocm's
struct NcclConfig214 {
  size_t size = sizeof(NcclConfig214);
  unsigned magic = 0xcafebeef;
  unsigned version = 21400;  // NCCL_VERSION(2, 14, 0)
  int blocking = 0;          // non-blocking: ncclCommInitRankConfig returns at once, progress is polled
  int cgaClusterSize = (int)0x80000000, minCTAs = (int)0x80000000, maxCTAs = (int)0x80000000;  // UNDEF_INT
  const char* netName = nullptr;
};
struct Rccl {
  void* h = nullptr;
  int (*get_unique_id)(void*) = nullptr;                                   // ncclGetUniqueId
  int (*comm_init_rank)(void**, int, std::array<char, 128>, int) = nullptr;  // ncclCommInitRank
  int (*comm_init_rank_config)(void**, int, std::array<char, 128>, int, NcclConfig214*) = nullptr;
  int (*get_async_error)(void*, int*) = nullptr;                           // ncclCommGetAsyncError
  int (*comm_abort)(void*) = nullptr;                                      // ncclCommAbort
  int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*comm_destroy)(void*) = nullptr;
  int (*comm_finalize)(void*) = nullptr;                                   // ncclCommFinalize (optional)
  const char* (*error_string)(int) = nullptr;
  bool nonblocking() const { return comm_init_rank_config && get_async_error && comm_abort; }
};
constexpr int NCCL_FLOAT32 = 7, NCCL_SUM = 0, NCCL_IN_PROGRESS = 7;  // ncclFloat32, ncclSum, ncclInProgress

int rccl(Rccl** out) {
  static Rccl r;
  static bool tried = false;
  if (!tried) {
    tried = true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
      if (!r.h) r.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.h) break;
    }
    if (r.h) {
      r.get_unique_id = (int (*)(void*))dlsym(r.h, "ncclGetUniqueId");
      r.comm_init_rank = (int (*)(void**, int, std::array<char, 128>, int))dlsym(r.h, "ncclCommInitRank");
      r.comm_init_rank_config =
          (int (*)(void**, int, std::array<char, 128>, int, NcclConfig214*))dlsym(r.h, "ncclCommInitRankConfig");
      r.get_async_error = (int (*)(void*, int*))dlsym(r.h, "ncclCommGetAsyncError");
      r.comm_abort = (int (*)(void*))dlsym(r.h, "ncclCommAbort");
      r.all_reduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(r.h, "ncclAllReduce");
      r.comm_destroy = (int (*)(void*))dlsym(r.h, "ncclCommDestroy");
      r.comm_finalize = (int (*)(void*))dlsym(r.h, "ncclCommFinalize");
      r.error_string = (const char* (*)(int))dlsym(r.h, "ncclGetErrorString");
    }
  }
  if (!r.h || !r.get_unique_id || !r.comm_init_rank || !r.all_reduce || !r.comm_destroy)
    return fail(SMAML_ESTATE, "librccl not found (dlopen librccl.so.1)");
  *out = &r;
  return SMAML_OK;
}

int nccl_fail(Rccl* r, int rc, const char* what) {
  return fail(SMAML_EHIP, std::string(what) + ": " + (r->error_string ? r->error_string(rc) : std::to_string(rc)));
}

// A non-blocking communicator's call returned rc: wait (bounded) until its state leaves ncclInProgress.
// Returns the final state (0 = success), or -1 on timeout.
int nccl_wait(Rccl* r, void* comm, int rc, int64_t timeout_ms) {
  if (rc != NCCL_IN_PROGRESS || !comm || !r->get_async_error) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    int st = 0;
    const int q = r->get_async_error(comm, &st);
    if (q != 0) return q;
    if (st != NCCL_IN_PROGRESS) return st;
    if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() >
        timeout_ms)
      return -1;
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}
}  // namespace

extern "C" {

int smaml_comm_unique_id(uint8_t* id_out) {
  if (!id_out) return fail(SMAML_EINVAL, "id_out is NULL");
  Rccl* r = nullptr;
  TRY(rccl(&r));
  const int rc = r->get_unique_id(id_out);
  return rc ? nccl_fail(r, rc, "ncclGetUniqueId") : SMAML_OK;
}

// Bounded: with ncclCommInitRankConfig available the communicator is created non-blocking and its
// progress polled for at most comm_timeout_ms (smaml_set_option "comm_timeout_ms", default 120 s), so a
// rank whose peers never arrive (one of them failed before or inside its init) returns SMAML_EHIP
// instead of blocking forever; the half-built communicator is aborted.
int smaml_comm_init(smaml_ctx* c, int32_t rank, int32_t world, const uint8_t* id) {
  if (!c || !id || world < 1 || rank < 0 || rank >= world) return fail(SMAML_EINVAL, "bad comm_init arguments");
  if (c->comm) return fail(SMAML_ESTATE, "communicator already initialised");
  Rccl* r = nullptr;
  TRY(rccl(&r));
  TRY(ensure_device(c));
  std::array<char, 128> uid;
  std::memcpy(uid.data(), id, 128);
  void* comm = nullptr;
  if (r->nonblocking()) {
    NcclConfig214 cfg;
    int rc = r->comm_init_rank_config(&comm, world, uid, rank, &cfg);
    if (rc != 0 && rc != NCCL_IN_PROGRESS) {
      if (comm) (void)r->comm_abort(comm);
      return nccl_fail(r, rc, "ncclCommInitRankConfig");
    }
    rc = nccl_wait(r, comm, NCCL_IN_PROGRESS, c->comm_timeout_ms);
    if (rc != 0) {
      if (comm) (void)r->comm_abort(comm);
      if (rc < 0)
        return fail(SMAML_EHIP, "ncclCommInitRankConfig: timed out after " + std::to_string(c->comm_timeout_ms) +
                                    " ms waiting for the other ranks (communicator aborted)");
      return nccl_fail(r, rc, "ncclCommInitRankConfig");
    }
    c->comm_nb = 1;
  } else {
    const int rc = r->comm_init_rank(&comm, world, uid, rank);
    if (rc) return nccl_fail(r, rc, "ncclCommInitRank");
    c->comm_nb = 0;
  }
  c->comm = comm;
  return SMAML_OK;
}

int smaml_comm_allreduce(smaml_ctx* c, void* stream, float* buf, int64_t n) {
  if (!c || !buf || n < 0) return fail(SMAML_EINVAL, "bad allreduce arguments");
  if (!c->comm) return fail(SMAML_ESTATE, "smaml_comm_init not called");
  Rccl* r = nullptr;
  TRY(rccl(&r));
  TRY(ensure_device(c));
  int rc = r->all_reduce(buf, buf, (size_t)n, NCCL_FLOAT32, NCCL_SUM, c->comm, (hipStream_t)stream);
  if (c->comm_nb) rc = nccl_wait(r, c->comm, rc, c->comm_timeout_ms);  // enqueue completes (not the collective)
  if (rc < 0) return fail(SMAML_EHIP, "ncclAllReduce: enqueue timed out");
  return rc ? nccl_fail(r, rc, "ncclAllReduce") : SMAML_OK;
}

int smaml_comm_destroy(smaml_ctx* c) {
  if (!c) return fail(SMAML_EINVAL, "ctx is NULL");
  if (!c->comm) return SMAML_OK;
  Rccl* r = nullptr;
  TRY(rccl(&r));
  void* comm = c->comm;
  c->comm = nullptr;
  if (c->comm_nb && r->comm_finalize) {
    // non-blocking protocol: finalize (flushes outstanding work, reports its errors), poll it to completion
    // under the same bound as the init, then destroy; a finalize that never completes is aborted
    int rc = nccl_wait(r, comm, r->comm_finalize(comm), c->comm_timeout_ms);
    if (rc != 0) {
      (void)r->comm_abort(comm);
      if (rc < 0)
        return fail(SMAML_EHIP, "ncclCommFinalize: timed out after " + std::to_string(c->comm_timeout_ms) +
                                    " ms (communicator aborted)");
      return nccl_fail(r, rc, "ncclCommFinalize");
    }
  }
  int rc = r->comm_destroy(comm);
  if (c->comm_nb && rc == NCCL_IN_PROGRESS) rc = 0;  // (after finalize the destroy only frees resources)
  return rc ? nccl_fail(r, rc, "ncclCommDestroy") : SMAML_OK;
}

}  // extern "C"
