/*
 * smaml.h -- C ABI of libsmaml.so, the MI355X (gfx950) STGCN-LSTM MAML hot path.
 *
 * The reference (Yalt8826/WeatherForecast_STGCN_MAML) is pure Python with no FFI layer;
 * its boundary for this path is the module API of model.py / hybrid_model.py and the
 * train loop entry points of train_hybrid_maml_v5.py. Each entry point below names the
 * reference interface it replaces. The Python host package
 * (weatherforecast_stgcn_maml_amd/_capi.py) binds these with ctypes; INTEGRATION.md
 * shows the binding.
 *
 * Conventions
 *  - Every function returns an int status: 0 = OK, else an SMAML_E* code;
 *    smaml_last_error() returns the message of the calling thread's last failure.
 *  - Device buffers are caller-owned device pointers (e.g. torch tensors' data_ptr()),
 *    fp32, contiguous. Host arrays are marked _host.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream). All work is
 *    enqueued on it; no call synchronises the device unless documented.
 *  - A context is bound to one GPU, is not thread-safe, and is driven by one host thread.
 *  - Trainable parameters (LSTM + head, the only tensors that receive gradients: SURVEY
 *    F2) live in one flat "theta" vector in state_dict order; smaml_param_layout gives
 *    each tensor's offset (offsets are padded to 64 floats; pads must be zero).
 */
#ifndef SMAML_H
#define SMAML_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMAML_OK 0
#define SMAML_EINVAL 1   /* bad argument / shape */
#define SMAML_EHIP 2     /* HIP runtime error */
#define SMAML_ENOMEM 3   /* device allocation failed */
#define SMAML_ESTATE 4   /* missing set_graph / set_gcn_params / reserve / set_tasks */
#define SMAML_ENOTIMPL 5 /* requested mode not built */

typedef struct smaml_ctx smaml_ctx;

/* Model shapes: model.STGCN(...) (model.py:8-28) + HybridSTGCN_LSTM(...) (hybrid_model.py:16-58).
 *
 * Two sets of rules. smaml_create / smaml_param_layout accept what the GCN entry points
 * (smaml_gcn_conv*, smaml_gcn_forward, smaml_relu_mask, smaml_dropout) can run: every dimension positive,
 * input_channels and hidden_channels multiples of 4, lstm_hidden_size 32 / 64 / 128 / 256,
 * lstm_num_layers <= 8, forecast_horizon * output_channels <= 128, output_channels <= input_channels.
 * Every entry point that launches the LSTM or the head (smaml_forward, smaml_backward, smaml_backward_base, smaml_lstm_forward,
 * smaml_lstm_backward, smaml_head_loss, smaml_meta_step, smaml_inner_loop, smaml_adapt_prepare[_multi],
 * smaml_adapt_steps[_multi, _full], smaml_forecast, smaml_forecast_ensemble, smaml_forecast_rollout[_ensemble]) requires in addition
 *   hidden_channels % 16 == 0                        (the layer-0 K segment of the gate-GEMM tile loaders)
 *   (forecast_horizon * output_channels) % 4 == 0    (16-byte reads of prediction rows)
 * and returns SMAML_EINVAL naming the dimension otherwise, before it allocates or launches anything. */
typedef struct smaml_dims {
  int32_t num_nodes;         /* N: grid nodes per region (441 = 21x21) */
  int32_t window_size;       /* T (24); any positive length */
  int32_t input_channels;    /* 24 (multiple of 4) */
  int32_t hidden_channels;   /* GCN hidden (256): multiple of 4; of 16 for the LSTM / head entry points */
  int32_t lstm_hidden_size;  /* 128 (32, 64, 128 or 256) */
  int32_t lstm_num_layers;   /* 4 (1 .. 8) */
  int32_t forecast_horizon;  /* 8 */
  int32_t output_channels;   /* 12 (Hf*C <= 128; a multiple of 4 for the LSTM / head entry points) */
} smaml_dims;

const char* smaml_last_error(void);
int32_t smaml_abi_version(void);
/* Build description: the product form of each GEMM family (bf16x6 = each f32 operand split into
 * three bf16 pieces, six piece products on v_mfma_f32_32x32x16_bf16 accumulated in f32; or the
 * f32 MFMA). Host-only, no GPU needed. */
const char* smaml_build_info(void);

/* ---- host-only helpers (no GPU needed) ------------------------------------------ */

/* Flat layout of the trainable vector (which=0: lstm.* then output_layer.*, the order of
 * HybridSTGCN_LSTM.get_trainable_parameters(), hybrid_model.py:119-124) or of the frozen
 * GCN vector (which=1: base_stgcn.conv{1..4}.{bias,lin.weight}). Writes up to `cap`
 * offsets/sizes, *count tensors and *total padded floats. */
int smaml_param_layout(const smaml_dims* dims, int32_t which, int64_t* offsets, int64_t* sizes,
                       int32_t cap, int32_t* count, int64_t* total);

/* Normalised t=0 adjacency of PyG gcn_norm as ELL (width 8): replaces the
 * add_remaining_self_loops + degree + norm part of GCNConv (model.py:23-26) for the
 * edge_index of graphBuilder.build_spatial_graph (graphBuilder.py:9-47). Any edge_index with
 * in-degree <= 7 (self loops not counted) is accepted: parallel edges count twice, self loops in the
 * input are replaced by the one every node gets, isolated nodes keep that loop alone (weight 1), the
 * edge order is free. A source or target outside [0, num_nodes) or an in-degree of 8: SMAML_EINVAL
 * (smaml_graph_csr / smaml_set_graph_weighted take such graphs, and edge weights). */
int smaml_graph_ell(const int64_t* edge_index_host, int64_t num_edges, int32_t num_nodes,
                    int32_t* cols_host, float* vals_host);

/* The same adjacency as CSR, for any in-degree and optional edge weights (PyG 2.x gcn_norm with edge_weight;
 * host-only, the twin of smaml_graph_ell). edge_index [2, E] (sources, then targets), edge_weight [E] or NULL
 * (all ones):
 *  - an edge s -> t with s != t adds an entry of weight w_e to row t; parallel edges stay separate entries, so
 *    their contributions add;
 *  - self loops in the input are removed and every node gets one loop (add_remaining_self_loops): its weight is
 *    that of the LAST input entry (i, i) in edge order, 1 if there is none (NULL weights: always 1);
 *  - deg[t] = loop[t] + the sum of t's in-edge weights, summed in double in edge order, rounded once to float;
 *    dinv[t] = 1.f / sqrtf(deg[t]), 0 where deg[t] is 0; an entry's value is (dinv[s] * w) * dinv[t] in float;
 *  - row t holds its in-edges in input order, then its self loop; entries of value 0 (zero weights, anything
 *    touching a node of degree 0) are dropped. With NULL weights and in-degree <= 7 the rows are the ELL's
 *    non-padding columns and values, bit for bit.
 * SMAML_EINVAL, with a message naming the edge, before anything is written: an index outside [0, num_nodes), a
 * negative, NaN or infinite weight, more than 2^31 - 1 entries. rowptr_host [num_nodes + 1]; cols_host / vals_host
 * hold cap entries. *nnz_out is always written (0 if the graph is rejected); cap < *nnz_out: SMAML_EINVAL, with
 * rowptr, cols and vals untouched. */
int smaml_graph_csr(const int64_t* edge_index_host, const float* edge_weight_host, int64_t num_edges,
                    int32_t num_nodes, int32_t* rowptr_host, int32_t* cols_host, float* vals_host, int64_t cap,
                    int64_t* nnz_out);

/* ---- context ----------------------------------------------------------------------- */
int smaml_create(const smaml_dims* dims, int32_t device, smaml_ctx** out);
int smaml_destroy(smaml_ctx* ctx);

/* Upload the graph (edge_index [2, E] int64, host). */
int smaml_set_graph(smaml_ctx* ctx, const int64_t* edge_index_host, int64_t num_edges);

/* Upload the graph in its general form (smaml_graph_csr's rules: any in-degree, edge_weight_host [E] or NULL):
 * A_hat and A_hat^T as CSR. It replaces the context's graph exactly as smaml_set_graph does (the adaptation
 * feature cache is dropped, pending state stays as valid as it was) and every entry point that reads the graph
 * honours it; a later smaml_set_graph switches back to the ELL, and the other way round. A call of either that
 * fails leaves the live graph as it was. On a graph both accept the two forms give the same bits. */
int smaml_set_graph_weighted(smaml_ctx* ctx, const int64_t* edge_index_host, const float* edge_weight_host,
                             int64_t num_edges);

/* Host counters of the live graph (cap entries written, *count = 5): [0] form (0 none, 1 ELL, 2 CSR), [1] entries
 * of A_hat, [2] its longest row, and since the graph was set: [3] k_gcn_layer launches that gathered through the
 * CSR, [4] k_gather_rows / k_gcn_dz launches that read a CSR of A_hat or A_hat^T of the CSR form. */
int smaml_graph_stats(const smaml_ctx* ctx, int64_t* counts, int32_t cap, int32_t* count);

/* ---- weighted loss and weighted forecast scores -------------------------------------
 * Training loss. A table holds nsets sets, each [Hf*N][C] floats in the layout of the targets y (row h'*N + n',
 * column c). With a table the loss of every entry point below is inv * sum w (pred - y)^2 with the unchanged
 * inv = 1 / (B * N * Hf * C): the library does not normalise (scale a table to mean 1 and losses, clip thresholds
 * and learning rates keep their meaning). Per element, in f32: wd = w (p - y), loss += wd (p - y),
 * dpred = dscale wd, and in the second-order sweep R dpred = dscale (w R p). Where w == 0 the element contributes
 * exactly +0 to the loss, dpred and R dpred whatever y holds (NaN and infinity included); an all-ones table gives
 * bitwise the results of no table.
 * Which set a task reads: set 0 if nsets == 1; else the set with the task's index in the current smaml_set_tasks
 * list: task z of smaml_meta_step / smaml_inner_loop reads set z, region r of smaml_adapt_steps_multi reads set
 * tasks_host[r]; smaml_adapt_steps, smaml_adapt_steps_full and smaml_head_loss read set 0. With nsets > 1 and
 * nsets != the number of registered tasks, smaml_meta_step, smaml_inner_loop and the smaml_adapt_steps* calls
 * return SMAML_ESTATE naming both numbers before they launch anything.
 * Scores. One node weight vector v[N] multiplies every summand of smaml_forecast [0..2], smaml_forecast_rollout
 * [0..2], smaml_forecast_ensemble [0..3] and smaml_forecast_rollout_ensemble [0..3] by v[n'] of its target node,
 * (v e) e for the squared terms, v |e|, v var and v CRPS for the others, the rollouts' gap rows included; v == 0
 * gives exactly 0 whatever the target holds, all ones the unweighted bits. The fixed-order block and double sums
 * are unchanged; pred, traj, mean, spread and member_* are not affected.
 * State. Both tables survive smaml_set_tasks, smaml_set_graph[_weighted], smaml_set_gcn_params and smaml_reserve.
 * Setting or clearing them drops no cache (the adaptation feature cache does not depend on the loss) and leaves a
 * pending smaml_forward / smaml_backward pair valid. The caller does not set them while work that reads them is
 * in flight, as for smaml_set_graph. smaml_set_dropout composes with them unchanged. */
/* host-only: SMAML_EINVAL naming set and element for a negative, NaN or infinite weight, a set with no positive
 * weight, nsets <= 0, w_host NULL. */
int smaml_loss_weights_check(const smaml_dims* dims, const float* w_host, int32_t nsets);
/* copies [nsets][Hf*N][C] into a buffer the context owns (freed by smaml_destroy); runs the check above first and
 * leaves the live table alone if it fails; (NULL, 0) clears. Complete on return. */
int smaml_set_loss_weights(smaml_ctx* ctx, const float* w_host, int32_t nsets);
/* node weights [N] of the forecast score sums; same checks; NULL clears. */
int smaml_set_score_weights(smaml_ctx* ctx, const float* node_w_host);
/* (cap entries written, *count = 6) [0] loss sets held, [1] 1 if score weights are held, and since the last
 * set/clear of either: [2] weighted k_head_loss launches, [3] weighted k_head_loss_small, [4] weighted k_head_dual,
 * [5] weighted score launches. */
int smaml_loss_stats(const smaml_ctx* ctx, int64_t* counts, int32_t cap, int32_t* count);

/* Frozen GCN parameters (flat, layout which=1), device pointer kept by reference. */
int smaml_set_gcn_params(smaml_ctx* ctx, const float* gcn_flat);

/* The meta-step's per-stream GCN feature cache (option "gcn_stream_cache", default 1): with the frozen base and
 * no GCN dropout, smaml_meta_step computes the features of each stream row once and keeps them, per stream
 * (keyed by its device pointer and length), across inner steps, meta-steps and smaml_set_tasks calls.
 * smaml_set_gcn_params and smaml_set_graph[_weighted] forget the cached rows themselves. A caller who CHANGES
 * WHAT A REGISTERED STREAM'S MEMORY HOLDS -- writes it in place, or frees it and lets another stream of the same
 * length take its address -- must call this before the next smaml_meta_step: the cached rows are forgotten, the
 * tables stay allocated. Option "gcn_stream_cache_mb": cap on the tables' bytes (-1, the default: free HBM only). */
int smaml_gcn_cache_invalidate(smaml_ctx* ctx);

/* Size the workspace for `tasks` x `batch` samples per step (grows, never shrinks). */
int smaml_reserve(smaml_ctx* ctx, int32_t tasks, int32_t batch);

/* Bytes of device workspace currently held. */
int64_t smaml_workspace_bytes(const smaml_ctx* ctx);

/* Inner steps whose primal activations the last second-order smaml_meta_step kept for its
 * meta-backward sweep (tangent-only dual kernels there; the rest are recomputed). Sized to
 * free HBM, capped by smaml_set_option("keep") / the SMAML_KEEP environment variable. New; no reference counterpart. */
int32_t smaml_so_kept_steps(const smaml_ctx* ctx);

/* Train-mode dropout of smaml_meta_step / smaml_adapt_steps (replaces the nn.Dropout calls at
 * hybrid_model.py:67,70,73 (p_gcn = STGCN dropout_rate), the nn.LSTM inter-layer dropout
 * hybrid_model.py:42-49 and the head input dropout :108 (p_lstm = lstm_dropout)). Masks are
 * counter-based (seed, global task id, inner step, site, element), identical in the
 * forward, the backward and the second-order sweep; p = 0 (the default) disables them.
 * The reference draws masks from torch's RNG, so runs agree with it only at p = 0. */
int smaml_set_dropout(smaml_ctx* ctx, float p_gcn, float p_lstm, uint32_t seed);

/* Global task id of each task of the next smaml_set_tasks batch (the dropout masks' task
 * index, so a task's masks do not depend on how tasks are grouped or sharded). */
int smaml_set_task_ids(smaml_ctx* ctx, const int32_t* ids_host, int32_t n);

/* ---- forward (module API) ----------------------------------------------------------- */

/* GCNConv.forward(x, edge_index) (PyG semantics, F3): x [rows, cin] -> out [rows, cout].
 * Rows < num_nodes aggregate over the graph, the rest see only their self loop.
 * Short inputs: rows < num_nodes is SMAML_EINVAL ("rows ... must be at least num_nodes"), checked before
 * anything is launched -- row q < num_nodes gathers any of rows 0 .. num_nodes - 1 of x, so a shorter x would
 * be read past its end (PyG raises an IndexError there). */
int smaml_gcn_conv(smaml_ctx* ctx, void* stream, const float* x, int32_t rows, int32_t cin,
                   const float* weight, const float* bias, int32_t cout, float* out);

/* GCNConv / Linear forward and backward for the module API's autograd (model.py:7-52: STGCN trained on
 * its own; the hybrid path keeps the GCN frozen, F2). flags: SMAML_GCN_RELU applies ReLU to the output,
 * SMAML_GCN_PLAIN skips the graph aggregation (a plain x W^T + b, e.g. STGCN.output_layer).
 * Short inputs: without SMAML_GCN_PLAIN, rows < num_nodes is SMAML_EINVAL as in smaml_gcn_conv (nothing is
 * launched); with it any rows > 0 are accepted, since no row is gathered. */
#define SMAML_GCN_RELU 1
#define SMAML_GCN_PLAIN 2
int smaml_gcn_conv_ex(smaml_ctx* ctx, void* stream, const float* x, int32_t rows, int32_t cin,
                      const float* weight, const float* bias, int32_t cout, int32_t flags, float* out);

/* Backward of z = A_hat x W^T + b (SMAML_GCN_PLAIN: A_hat = I) given dz = dL/dz [rows][cout]:
 * dx = A_hat^T dz W [rows][cin] (optional), dwb = [dL/dW (cout x cin, row-major) | dL/db (cout)]
 * (optional). Deterministic (fixed-order sums). Replaces autograd through PyG GCNConv / nn.Linear.
 * Short inputs: without SMAML_GCN_PLAIN, rows < num_nodes is SMAML_EINVAL as in smaml_gcn_conv (both the
 * A_hat x of dW and the A_hat^T dz of dx gather rows 0 .. num_nodes - 1); nothing is launched or reserved. */
int smaml_gcn_conv_backward(smaml_ctx* ctx, void* stream, const float* x, int32_t rows, int32_t cin,
                            const float* weight, int32_t cout, const float* dz, int32_t flags, float* dx, float* dwb);

/* g *= (h > 0) over n elements: the ReLU derivative from the post-activation h (F.relu's backward). */
int smaml_relu_mask(smaml_ctx* ctx, void* stream, float* g, const float* h, int64_t n);

/* HybridSTGCN_LSTM.forward(x, edge_index) (hybrid_model.py:80-117) for `nsamples` samples:
 * x_host[s] = device pointer to sample s's x [T*N, input_channels] (time-major rows);
 * pred [nsamples][N*Hf][C] (rows n*Hf + h); feats (optional) [nsamples][T*N][Hc] = the
 * extract_base_features output (hybrid_model.py:60-78). With smaml_set_dropout p > 0 this is the
 * train-mode forward (masks of (seed, task id 0 of smaml_set_task_ids, step 0)); the following
 * smaml_backward applies the same masks. */
int smaml_forward(smaml_ctx* ctx, void* stream, const float* theta, const float* const* x_host,
                  int32_t nsamples, float* pred, float* feats);

/* ---- training ------------------------------------------------------------------------ */

/* Register the tasks' feature streams: features_host[j] = device pointer to a
 * [t_total[j], N, input_channels] stream (WeatherGraphDataset.features, dataset.py:6-25).
 * A sample is addressed by its window start w: x = stream[w:w+T], targets
 * stream[w+T+1 .. w+T+Hf, :, :C] (dataset.py:30-48, F5). */
int smaml_set_tasks(smaml_ctx* ctx, int32_t ntasks, const float* const* features_host,
                    const int32_t* t_total_host);

/* Rolling forecast over a registered stream: what validate_hybrid_v5.validateAdapted's no-grad forward
 * (validate_hybrid_v5.py:189-237) and adaptModel's validation loop (adapt_hybrid_v5.py:216-231) compute,
 * for any number of windows and, without `skill`, past the end of the stream. Runs the `nwin` windows
 * (starts windows_host[i]) of task `task` of smaml_set_tasks in passes of at most `batch` windows with
 * theta (one flat trainable vector), in eval mode (smaml_set_dropout does not apply).
 *   A window needs w >= 0 and w + T <= t_total (its inputs); with `skill` also w + T + Hf < t_total (its
 *   targets): otherwise SMAML_EINVAL naming the window. pred and skill both NULL: SMAML_EINVAL.
 *   pred (device, optional) [nwin][N*Hf][C]: normalised predictions, rows n*Hf + h as smaml_forward.
 *   skill (device doubles, optional) [3][Hf][C], overwritten: per target lead h' and variable c, over all
 *   windows and nodes, with the F4 pairing of the training loss (flat prediction row r = n*Hf + h is
 *   compared with target (h' = r / N, n' = r % N)):
 *     [0] sum (s_c (p - y))^2, [1] sum |s_c (p - y)|, [2] sum (s_c (y_last - y))^2 (persistence),
 *   y = stream[w+T+1+h', n', c], y_last = stream[w+T-1, n', c], s_c = scale_host[c] (NULL = 1; e.g. the
 *   adaptation checkpoint's std, giving physical units -- the mean cancels). Fixed-order sums (f32 per
 *   block, double across blocks and passes): bitwise repeatable.
 * The LSTM runs an inference-only step (k_lstm_fwd_infer) that keeps h and c of the two most recent
 * steps per layer instead of the activations a backward needs. A pass of consecutive windows
 * (w[b] = w[0] + b, more than one) computes the GCN features and layer 0's input projection once per
 * distinct stream row (options gcn_dedup / xg_dedup / f_compact); other passes compute per window.
 * Buffers are the forecast's own, sized from the pass size (they grow, never shrink; smaml_forecast_bytes):
 * the call does not go through smaml_reserve, leaves smaml_workspace_bytes, the adaptation feature cache
 * and the state of smaml_meta_step alone, and a pending smaml_forward / smaml_backward (or smaml_lstm_
 * forward / _backward) pair STAYS VALID across it: the backward may follow a forecast. */
int smaml_forecast(smaml_ctx* ctx, void* stream, const float* theta, int32_t task, const int32_t* windows_host,
                   int32_t nwin, int32_t batch, const float* scale_host, float* pred, double* skill);

/* Bytes of device memory the forecast's own buffers hold (not part of smaml_workspace_bytes; those of
 * smaml_forecast_ensemble, smaml_forecast_rollout and smaml_forecast_rollout_ensemble included). */
int64_t smaml_forecast_bytes(const smaml_ctx* ctx);

/* Autoregressive rollout: the forecast fed back in, to reach lead times past the model's Hf steps. New; the
 * reference forecasts one horizon per window only. Stride s = Hf + 1.
 *   Origin o (a window start in task `task`'s stream S) gets a private sequence X, rows [N][Cin]:
 *   X[rho] = S[o + rho] for rho < T. Cycle j = 0 .. R-1 (R = `cycles`): the window is X[j s : j s + T]; the
 *   eval-mode output is P flat [N*Hf][C], read as [Hf][N][C] -- the F4 pairing the model was trained with
 *   (flat row r is lead h' = r / N, node n' = r % N). With rho0 = j s + T the cycle appends
 *     X[rho0 + 1 + h'][n'][c] = P[h'][n'][c]                                  for c < C,
 *     X[rho0][n][c] = 0.5f * (X[rho0 - 1][n][c] + P[0][n][c]) in f32          gap = 1 (midpoint), or
 *     X[rho0][n][c] = X[rho0 - 1][n][c]                                       gap = 0 (persistence):
 *   the targets skip t + 0 (F5), so row rho0 is a gap no forecast covers. Channels c >= C of every appended
 *   row are S[o + rho][n][c]: the caller registers a stream whose rows past the last observation carry valid
 *   exogenous (calendar, Koppen) channels; the weather channels of those rows are never read as inputs and
 *   may be NaN.
 *   Checked before anything is allocated or launched (SMAML_EINVAL naming the origin): o >= 0,
 *   o + T + (R - 1) s <= t_total, with `skill` o + T + R s <= t_total. traj and skill both NULL, cycles <= 0,
 *   gap outside {0, 1}, norig or batch <= 0: SMAML_EINVAL before a context or device is needed.
 *   traj (device, optional) [norig][R][s][N][C], normalised: the weather channels of the appended rows; row 0
 *   of each cycle is the gap row, rows 1..Hf the memory image of P, bit for bit.
 *   skill (device doubles, optional) [3][R s][C], overwritten: per absolute lead k = j s + i and variable,
 *   sums over origins and nodes of every traj row x against y = S[o + T + k]:
 *     [0] sum (s_c (x - y))^2, [1] sum |s_c (x - y)|, [2] sum (s_c (y_last - y))^2, y_last = S[o + T - 1],
 *   s_c = scale_host[c] (NULL = 1). Fixed order as smaml_forecast's sums (f32 per block, double across blocks
 *   and passes): bitwise repeatable.
 * The origins run in passes of at most `batch`; all origins of a pass advance in lockstep through the R cycles.
 * The private sequences live on the device and k_rollout_append writes each cycle's rows into them (one launch
 * per cycle over the pass), so nothing is copied or uploaded between cycles: one pointer table per call. Layer
 * 0's input projection is kept across cycles in a slot table [S][M][4H] (M = B N; private row rho in slot
 * rho % S, S = T) that k_lstm_fwd_infer reads through XgDedup's second addressing mode; per cycle only the rows
 * the previous cycle appended go through the position-independent GCN (the row-run form of k_gcn_mlp, or the
 * per-layer kernels) and the projection, while the window's t = 0 rows, whose features aggregate over the graph
 * (F3), are recomputed every cycle into a block of their own. smaml_set_option("roll_reuse", 0) recomputes
 * every row of every window each cycle through the same kernels into the same table: bitwise the same results.
 * State isolation as smaml_forecast: buffers of its own (grow only, in smaml_forecast_bytes), the workspace, the
 * adaptation cache and the meta-step state untouched, a pending smaml_forward / smaml_backward pair stays
 * valid, eval mode, no stream synchronisation. */
int smaml_forecast_rollout(smaml_ctx* ctx, void* stream, const float* theta, int32_t task,
                           const int32_t* origins_host, int32_t norig, int32_t batch, int32_t cycles, int32_t gap,
                           const float* scale_host, float* traj, double* skill);

/* Host-side counters of the last smaml_forecast_rollout call that passed its checks, summed over its passes; a
 * "row" is one time step of one origin (N node rows): [0] cycles run, [1] rows whose GCN features the
 * position-independent path computed (per origin (T - 1) + (R - 1) min(s, T - 1) with roll_reuse, R (T - 1)
 * without), [2] rows through the t = 0 graph path (one per origin and cycle), [3] rows of layer-0 projection
 * computed ([1] + [2]), [4] append launches. Writes min(cap, count) entries; *count = 5. Measurement and tests. */
int smaml_rollout_stats(const smaml_ctx* ctx, int64_t* counts, int32_t cap, int32_t* count);

/* MC-dropout ensemble forecast: `members` (E, 1..64) stochastic forwards per window, in lockstep over the
 * member axis, with the ensemble mean, spread and probabilistic scores. Windows, passes, alignment and
 * range errors as smaml_forecast. Member e of window i (position in windows_host) is what
 * HybridSTGCN_LSTM.train()'s forward under no_grad computes for that window with this library's
 * counter-based masks (kernels.h Drop; oracle/refcpu.py Dropout):
 *   Masks: member e uses the sites drop_site(seed, kind, step = e, layer) with task id 0. The probabilities
 *   (p_gcn: after conv1..conv3; p_lstm: between LSTM layers and on the head input; each in [0, 1), 0 = that
 *   site off) and the seed are this call's arguments: the state of smaml_set_dropout / smaml_set_task_ids
 *   is neither read nor changed.
 *   Element indices are those of the training forward of ONE batch holding the whole window list:
 *   B := nwin, sample b := i, M := nwin*N, row m := i*N + n:
 *     kind 1, layer k:  ((0*nwin + i) * T*N + row) * Hc + ch      (row = t*N + n of the window)
 *     kind 2, layer l:  ((0*T + t) * nwin*N + i*N + n) * H + unit
 *     kind 3:           (i*N + n) * H + unit
 *   so a member does not depend on `batch`, on how the list is cut into passes or on the grouping below, and
 *   refcpu.batch_loss(Pt, Pg, task, windows, refcpu.Dropout(seed, p_gcn, p_lstm, 0, e)) is member e's oracle.
 *   SMAML_EINVAL (with a message): members outside 1..64; a probability outside [0, 1); mean, spread,
 *   member_pred and scores all NULL; scores requested for a window without targets; smaml_forecast's errors.
 *   member_pred (device, optional) [members][nwin][N*Hf][C]: normalised predictions, rows n*Hf + h.
 *   mean, spread (device, optional) [nwin][N*Hf][C]: the member sum in member order divided by E; the
 *   unbiased standard deviation about that mean (two-pass), 0 when E = 1.
 *   scores (device doubles, optional) [4][Hf][C], overwritten: sums over windows and nodes with the F4
 *   pairing, y, y_last and s_c = scale_host[c] exactly as smaml_forecast's skill sums:
 *     [0] sum (s (mu - y))^2          the error of the ensemble mean
 *     [1] sum s^2 sigma^2             the unbiased ensemble variance
 *     [2] sum s CRPS,  CRPS = (1/E) sum_i |x_i - y| - (1/(2 E^2)) sum_{i,j} |x_i - x_j|
 *                                     (formed as (1/E^2) sum_{i<j}, the pairs in lexicographic order)
 *     [3] sum (s (y_last - y))^2      persistence
 *   Fixed order: f32 per block, double across blocks and passes. Bitwise repeatable.
 * What does not depend on the masks runs once per pass: with p_gcn == 0 the GCN features and layer 0's input
 * projection (per distinct stream row on consecutive windows, as smaml_forecast) and layer 0 of the LSTM
 * itself when a layer above reads it, i.e. with two or more LSTM layers (option ens_share, default 1; 0
 * computes it per member: bitwise the same members; a one-layer LSTM always does). With p_gcn > 0
 * every member runs its own GCN. Members run ens_group at a time (option; 0 = all, default -1 = the largest
 * group whose rings and per-member features fit 2 GiB); any grouping gives bitwise the same result.
 * State isolation as smaml_forecast: the buffers are the forecast's own (grow only, in smaml_forecast_bytes),
 * smaml_workspace_bytes, the adaptation feature cache and the meta-step state are untouched, and a pending
 * smaml_forward / smaml_backward pair stays valid across the call. */
int smaml_forecast_ensemble(smaml_ctx* ctx, void* stream, const float* theta, int32_t task,
                            const int32_t* windows_host, int32_t nwin, int32_t batch, int32_t members, float p_gcn,
                            float p_lstm, uint32_t seed, const float* scale_host, float* mean, float* spread,
                            float* member_pred, double* scores);

/* Ensemble rollout: `members` (E, 1..64) MC-dropout members, each fed its OWN forecast back in for `cycles`
 * (R, 1..1024) cycles -- how the ensemble spread grows with lead time. Notation as smaml_forecast_rollout:
 * s = Hf + 1, origin i = origins_host[i] in task `task`'s stream S.
 *   Member e of origin i keeps a private sequence X(e,i), X(e,i)[rho] = S[o_i + rho] for rho < T. Cycle j: the
 *   window is X(e,i)[j s : j s + T]; the output P(e,i) is what HybridSTGCN_LSTM.train()'s forward under no_grad
 *   computes on that window with this library's counter-based masks.
 *   Masks: the sites drop_site(seed, kind, step = 64 j + e, layer) with task id 0; the element indices are those
 *   of the training forward of ONE batch holding the whole origin list (B := norig, sample b := i, M := norig*N,
 *   row m := i*N + n): the three index lines of smaml_forecast_ensemble, t the step inside the window. Member
 *   e's oracle for cycle j is refcpu.stgcn_features(x_i, ei, Pg, drop, i, norig) per origin, then
 *   refcpu.batched_forward(P, feats, dims, drop), drop = refcpu.Dropout(seed, p_gcn, p_lstm, 0, 64*j + e). A member
 *   depends on none of: `batch`, how origins are cut into passes, the member grouping, E, R. Cycle 0 is by
 *   definition smaml_forecast_ensemble's member e on the window list `origins`. The probabilities and the seed are
 *   this call's arguments: smaml_set_dropout / smaml_set_task_ids are neither read nor written.
 *   Append: smaml_forecast_rollout's rule, per member from its own P(e,i): the gap row by midpoint (gap = 1) or
 *   persistence (gap = 0) in f32, then the Hf rows of P; channels c >= C from the stream.
 *   Checked before anything is allocated or launched, SMAML_EINVAL with a message; the first line before a
 *   context or device is needed: member_traj, mean, spread and scores all NULL; norig or batch <= 0; members
 *   outside 1..64; cycles outside 1..1024 (the mask site packs step << 8 below kind << 24, so the step
 *   64 j + e has 16 bits: 64 * 1023 + 63 = 65535 is the last that fits); a probability outside [0, 1); gap
 *   outside {0, 1}. Then, naming the origin: o >= 0, o + T + (R - 1) s <= t_total, with `scores`
 *   o + T + R s <= t_total.
 *   Outputs, all optional, on the device, normalised:
 *   member_traj [E][norig][R][s][N][C]: row 0 of a cycle is the gap row, rows 1..Hf the memory image of P.
 *   mean, spread [norig][R][s][N][C]: the member sum in member order divided by E; the unbiased standard
 *   deviation about that mean (two-pass, accumulated in double, rounded once), 0 at E = 1.
 *   scores (doubles) [4][R s][C], overwritten: per absolute lead k = j s + r and variable, sums over origins and
 *   nodes of every trajectory row (gap rows included) against y = S[o + T + k], s_c = scale_host[c] (NULL = 1):
 *     [0] sum (s_c (mu - y))^2     [1] sum s_c^2 sigma^2
 *     [2] sum s_c CRPS, CRPS = (1/E) sum_i |x_i - y| - (1/E^2) sum_{i<j} |x_i - x_j| (pairs in lexicographic order)
 *     [3] sum (s_c (y_last - y))^2, y_last = S[o + T - 1]
 *   Fixed order: f32 per block, double across blocks and passes, no atomics. Bitwise repeatable.
 * Origins run in passes of at most `batch`; within a pass the members run G at a time over grid z, every
 * (member, origin) pair of a group in lockstep through the R cycles. G = option ens_group (0 = all), default the
 * largest group whose rings, slot tables, sequences and features fit option roll_ens_budget_mb (floor 1). Any
 * grouping is bitwise equal. With p_gcn == 0 the eval-form GCN is position-independent: the observed rows
 * (rho < T) are the same in every member, so their features and layer-0 projection are computed once per pass
 * into a table all members read, and only the rows a member appended go through the GCN and projection per
 * member (option roll_reuse; 0 recomputes every row per member and cycle: bitwise equal). In cycle 0 all members
 * read the same window: its t = 0 graph block is computed once, and with two or more LSTM layers layer 0 runs
 * once (option ens_share); from cycle 1 on both are per member. With p_gcn > 0 the kind-1 masks depend on cycle
 * and position: every member recomputes all T rows each cycle on the per-layer kernels (correct, not tuned).
 * State isolation as the other forecast calls: buffers of its own (grow only, in smaml_forecast_bytes), the
 * workspace, the adaptation cache and the meta-step state untouched, a pending smaml_forward / smaml_backward
 * pair stays valid, no stream synchronisation. */
int smaml_forecast_rollout_ensemble(smaml_ctx* ctx, void* stream, const float* theta, int32_t task,
                                    const int32_t* origins_host, int32_t norig, int32_t batch, int32_t cycles,
                                    int32_t gap, int32_t members, float p_gcn, float p_lstm, uint32_t seed,
                                    const float* scale_host, float* member_traj, float* mean, float* spread,
                                    double* scores);

/* Host-side counters of the last smaml_forecast_rollout_ensemble call that passed its checks, summed over its
 * passes and member groups; a "row" is one time step of one origin (N node rows): [0] cycles run (one per group
 * and cycle), [1] member-rows through the position-independent GCN (with roll_reuse and p_gcn == 0:
 * E norig (R - 1) min(s, T - 1)), [2] shared rows through it (observed rows, once per pass: norig (T - 1)),
 * [3] rows through the t = 0 graph path, [4] rows of layer-0 projection computed ([1] + [2] + [3]; none at p_gcn > 0), [5] append launches,
 * [6] member groups run. Writes min(cap, count) entries; *count = 7. Measurement and tests. */
int smaml_rollout_ensemble_stats(const smaml_ctx* ctx, int64_t* counts, int32_t cap, int32_t* count);

/* One meta-step over all registered tasks (meta_update_v4, train_hybrid_maml_v5.py:144-184,
 * wrapping inner_loop_v4, :110-141):
 *   per task: fast = theta; for k < steps: B-sample support step (mean MSE, backward,
 *   clip_grad_norm_(max_norm), SGD(inner_lr)); then one B-sample query batch.
 * windows_host: int32 [(steps+1)][ntasks][batch] window starts (row `steps` = query).
 * order 0: reference semantics (the reference's outer step is a no-op):
 *          query loss only; order 1: first-order MAML meta-gradient; order 2: second-order.
 * meta_grad [P]: sum over tasks of d(query_scale * query_mse)/d(theta) (order >= 1).
 * losses [(steps+1)][ntasks]: per-step support MSE; last row = query MSE (unscaled).
 * norms [steps][ntasks] (optional): pre-clip gradient norms. fast_out [ntasks][P]
 * (optional): adapted parameters. */
int smaml_meta_step(smaml_ctx* ctx, void* stream, const float* theta, int32_t order, int32_t steps,
                    int32_t batch, const int32_t* windows_host, float inner_lr, float max_norm,
                    float query_scale, float* meta_grad, float* losses, float* norms, float* fast_out);

/* smaml_meta_step with the GCN base meta-trained too: the same call, plus the base's meta-gradient. The inner
 * loop is smaml_meta_step's -- every task adapts theta by clip + SGD; the base g is shared by the tasks and is
 * not adapted per task -- and meta_grad, losses, norms and fast_out are bitwise what smaml_meta_step writes for
 * the same arguments (one driver; the base work is added after the existing launches of the query step and of
 * each sweep step).
 *   gcn_meta_grad [Pg] (device, required, 16-byte aligned; layout of smaml_param_layout(which = 1)): overwritten,
 *     pads zero: sum over tasks of d(query_scale * L_q(fast_K(theta, g), g)) / dg.
 *   order 1: the partial derivative at the adapted parameters (fast_K held constant): one base backward on the
 *     query batch. order 2: the total derivative: each inner step k adds -inner_lr d(g_k . w_k)/dg, g_k that
 *     step's theta-gradient and w_k the clip-adjusted direction the sweep forms for theta's Hessian product (the
 *     clip's derivative included). The base has no theta-tangent, so the mixed term is the linear GCN backward
 *     of the tangent of the layer-0 input gradient, R dF_k = R dG0_k . W_ih0(theta_k) + dG0_k . U_ih0 (U = w_k's
 *     W_ih0 block), masked by conv4's ReLU derivative, through conv4..conv1 with step k's activations.
 *     order 0: SMAML_EINVAL.
 * The base stage runs once per query step and (order 2) once per sweep step, right after that step's backward:
 * k_lstm_dx0_meta forms the masked layer-0 input gradient of every task in one launch (tangent: one K loop over
 * [R dG0 | dG0] . [W_ih0 ; U_ih0]), conv1..conv3's outputs are recomputed from the step's windows, and conv4..
 * conv1 run smaml_gcn_conv_backward's launches per task. Two row forms, chosen per step:
 *   per-sample: T B N rows per task in smaml_backward_base's sample layout (scattered windows, batch 1,
 *     p_lstm > 0; every step with option "meta_base_dedup" = 0);
 *   distinct-row (steps whose tasks read consecutive windows, batch > 1, no dropout; option "meta_base_dedup",
 *     default 1): the (2B + T - 2) N distinct stream rows per task -- the B N rows of t = 0 as B samples on the
 *     graph path, stream rows w0 + 1 .. w0 + B + T - 2 as one neighbour-less block -- from the row sums of
 *     k_dg_rowsum (the ReLU mask and the sum over a stream row's window slots commute). Within tolerance of the
 *     per-sample form, not bitwise: the summation order differs.
 * Each task's (and block's) dW, db are written to a slot of their own and added in task order: deterministic
 * (fixed-order sums), bitwise repeatable. Loss weights and both graph forms compose. p_lstm > 0 is supported
 * (per-sample form). The stage's buffers are the context's own: they grow only and are freed by smaml_destroy.
 * Checks: smaml_meta_step's, plus order, gcn_meta_grad and meta_grad (SMAML_EINVAL, before a context is needed);
 * p_gcn > 0 (smaml_set_dropout): SMAML_ENOTIMPL before anything is allocated or launched. Every buffer is grown
 * before the first launch: SMAML_ENOMEM leaves all outputs untouched. Does not synchronise the stream. The caller
 * updates the base and calls smaml_set_gcn_params again (the per-stream feature cache forgets its rows).
 * Not covered: per-task base adaptation in the inner loop, p_gcn > 0, smaml_adapt_steps_multi with a trained base. */
int smaml_meta_step_base(smaml_ctx* ctx, void* stream, const float* theta, int32_t order, int32_t steps,
                         int32_t batch, const int32_t* windows_host, float inner_lr, float max_norm,
                         float query_scale, float* meta_grad, float* gcn_meta_grad, float* losses, float* norms,
                         float* fast_out);

/* Host-side counters of the last smaml_meta_step_base call that reached its buffers: [0] base stages run (order
 * 1: 1, order 2: 1 + steps), [1] of those, stages in the distinct-row form, [2] in the per-sample form, [3]
 * tangent stages, [4] bytes held by the stage's buffers, [5] rows sent through the GCN backward. Writes
 * min(cap, count) entries; *count = 6. Measurement and tests only. */
int smaml_meta_base_stats(const smaml_ctx* ctx, int64_t* counts, int32_t cap, int32_t* count);

/* Outer update (train_hybrid_maml_v5.py:174-179, 245-249): clip_grad_norm_(max_norm) of
 * `grad` then torch.optim.AdamW step `step` (1-based) on theta, m, v (n floats).
 * norm_out (optional, device float): pre-clip norm. */
int smaml_adamw_step(smaml_ctx* ctx, void* stream, float* theta, const float* grad, float* m, float* v,
                     int64_t n, int32_t step, float lr, float beta1, float beta2, float eps,
                     float weight_decay, float max_norm, float* norm_out);

/* Regional adaptation (adapt_hybrid_v5.adaptModel, adapt_hybrid_v5.py:182-203): `nsteps`
 * sequential fine-tuning steps on task 0 of smaml_set_tasks, each on `batch` windows
 * (windows_host [nsteps][batch]; the reference uses batch 1, shuffled): forward, MSE,
 * backward, clip_grad_norm_(max_norm), torch.optim.Adam with coupled L2 weight decay
 * (create_climate_optimizer, adaptive_scheduler.py:68-94) at learning rate lr_dev[k]
 * (device floats; ClimateAwareLRScheduler values) and Adam step step0+k+1.
 * theta, m, v: flat trainable vectors (device). losses [nsteps] (device): per-step MSE.
 * At batch 1 without GCN dropout each window's GCN features are cached on first use and reused
 * by later calls (frozen GCN): call smaml_set_gcn_params again after changing the GCN
 * parameters in place (it, smaml_set_graph and smaml_set_tasks drop the cache). */
int smaml_adapt_steps(smaml_ctx* ctx, void* stream, float* theta, float* m, float* v, int32_t step0,
                      int32_t nsteps, int32_t batch, const int32_t* windows_host, const float* lr_dev,
                      float beta1, float beta2, float eps, float weight_decay, float max_norm,
                      float* losses);

/* Set-up half of smaml_adapt_steps, for callers that keep allocation out of their timed epochs
 * (adaptModel builds its model and optimiser before the epoch loop, adapt_hybrid_v5.py:152-181):
 * sizes the workspace for `batch`-sample steps and allocates the per-window GCN feature cache
 * (batch 1), touching both once and synchronising `stream`. smaml_adapt_steps does the same on its
 * first call when this was not called. No compute; the cache stays cold. */
int smaml_adapt_prepare(smaml_ctx* ctx, void* stream, int32_t batch);

/* Several regions adapted in lockstep (main.py adapts its regions one after another; they are independent
 * problems of one shape): region r is task tasks_host[r] of smaml_set_tasks (distinct, in range), with
 * its own theta / m / v [nregions][P], learning rates lr_dev [nsteps][nregions] (device), weight decay
 * weight_decay_host [nregions] and windows windows_host [nsteps][nregions][batch] (starts into that
 * region's stream, validated against its length). For every k, step k of all regions runs as one set of
 * launches over the task axis; all regions share the Adam step step0+k+1. Region r computes what
 * smaml_adapt_steps computes on that stream alone with that region's theta, m, v, lr and weight decay
 * (one region: bitwise). losses [nsteps][nregions] (device). Nothing synchronises the stream; the
 * per-step tables are uploaded once per call. Every region has a GCN feature cache of its own (batch 1,
 * no GCN dropout); when one of them does not fit, all regions compute their GCN per step. Dropout masks
 * are keyed by each region's id of smaml_set_task_ids (all ids 0: the single-region masks in every
 * region). smaml_set_option("adapt_group", g) runs the regions g at a time (0 = all at once; default: see there). */
int smaml_adapt_steps_multi(smaml_ctx* ctx, void* stream, int32_t nregions, const int32_t* tasks_host,
                            float* theta, float* m, float* v, int32_t step0, int32_t nsteps, int32_t batch,
                            const int32_t* windows_host, const float* lr_dev, const float* weight_decay_host,
                            float beta1, float beta2, float eps, float max_norm, float* losses);
/* smaml_adapt_prepare for the regions of a lockstep call: the workspace and every region's feature cache. */
int smaml_adapt_prepare_multi(smaml_ctx* ctx, void* stream, int32_t nregions, const int32_t* tasks_host,
                              int32_t batch);

/* Host-timed phases of the last smaml_adapt_steps / smaml_adapt_steps_multi / smaml_adapt_steps_full call (the
 * last never fills a cache: [0] .. [2] stay 0 there), in ms: [0] workspace reserve, [1] feature-
 * cache allocation, [2] the batched feature-cache fill, [3] the step loop ([2] and [3] are enqueue
 * times unless smaml_set_option("adapt_phase_sync", 1), which ends each with a stream sync).
 * Writes min(cap, count) entries; *count = number of phases; *filled = windows whose features a
 * step computed itself (outside the batched fill). Measurement only; no reference counterpart. */
int smaml_adapt_phases(const smaml_ctx* ctx, double* ms, int32_t cap, int32_t* count, int64_t* filled);

/* Whole-model regional adaptation: smaml_adapt_steps with the GCN base trained too -- what the reference's
 * adaptation script announces (freeze_base=False, one optimiser "for ALL parameters (STGCN + LSTM)") and its
 * no_grad in extract_base_features withholds (F2). One region: task 0 of smaml_set_tasks. Step k: forward in
 * train mode (the masks of smaml_set_dropout, task id 0, step step0 + k), MSE, the backward through the head,
 * the LSTM and conv4..conv1, clip_grad_norm_(max_norm) over ALL gradients jointly (the trainable vector's and
 * the GCN vector's; squared sum in double, fixed order), torch.optim.Adam with coupled L2 weight decay at
 * lr_dev[k], Adam step step0 + k + 1, on both vectors (the element arithmetic of smaml_adapt_steps).
 *   theta, m, v [P] (layout which = 0) and gcn, gcn_m, gcn_v [Pg] (layout which = 1): device, 16-byte aligned,
 *     updated in place; the pads of both layouts stay zero.
 *   windows_host [nsteps][batch], lr_dev [nsteps], step0, losses [nsteps]: as smaml_adapt_steps. Any batch >= 1.
 *   norms (device, optional) [nsteps]: the joint gradient norm of each step before clipping.
 * gcn becomes the context's GCN parameter vector exactly as after smaml_set_gcn_params(gcn) (no earlier
 * smaml_set_gcn_params is needed), so a following smaml_forecast, smaml_meta_step(order 0), smaml_forward or
 * smaml_adapt_steps sees the adapted base. The batch-1 feature cache of smaml_adapt_steps is invalidated and
 * is neither allocated nor read here (it describes a frozen base). A pending smaml_forward / smaml_backward
 * pair is consumed. The forward keeps conv1..conv3's outputs for the backward (k_gcn_mlp's keep variant where
 * the fused GCN runs, else the per-layer launches write them in place), the layer-to-layer gradient is a GEMM,
 * a gather and a mask pass per layer (option "gcn_dz_fused" = 1: one GEMM with the mask in its epilogue plus a
 * gather over the t = 0 rows, k_gcn_dz), and the clip and Adam of both vectors are two launches (k_sqsum,
 * k_adam_l2 over two segments). Option "gcn_keep" = 0 recomputes the kept outputs instead. The kept activations and gradient buffers (batch*T*N rows x 5 Hc floats and smaller
 * pieces) are the context's own: they grow only and are freed by smaml_destroy.
 * Checked before anything is allocated or launched, the NULL arguments, alignment and counts before a device
 * is needed: NULL arguments (norms may be NULL), alignment, nsteps and batch positive, step0 non-negative
 * (SMAML_EINVAL); the dims of the LSTM path, the graph and the tasks (SMAML_EINVAL / SMAML_ESTATE); the window
 * range (SMAML_EINVAL). Every buffer is grown before the first launch: SMAML_ENOMEM leaves all six vectors
 * untouched. Deterministic (fixed-order sums); does not synchronise the stream.
 * Not covered: smaml_adapt_steps_multi with a trained base (the meta-step's base gradient: smaml_meta_step_base). */
int smaml_adapt_steps_full(smaml_ctx* ctx, void* stream, float* theta, float* m, float* v, float* gcn, float* gcn_m,
                           float* gcn_v, int32_t step0, int32_t nsteps, int32_t batch, const int32_t* windows_host,
                           const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                           float max_norm, float* losses, float* norms);

/* Host-side launch counters of the last smaml_adapt_steps_full call: [0] steps, [1] fused keeping-GCN launches
 * (k_gcn_mlp's keep variant), [2] per-layer keeping-GCN launches (k_gcn_layer over all rows writing conv k's
 * output where the backward reads it; the t = 0 launches beside the fused kernel are not counted), [3] fused
 * k_gcn_dz launches, [4] launches of the composed form (GEMM, gather, mask), [5] launches recomputing conv1..
 * conv3 (option "gcn_keep" = 0). Writes min(cap, count) entries; *count = 6. Measurement and tests only. */
int smaml_adapt_full_stats(const smaml_ctx* ctx, int64_t* counts, int32_t cap, int32_t* count);

/* ---- finer-grained operators (the module pieces callers compose) -------- */

/* Backward of the most recent smaml_forward (same theta): dpred [nsamples][N*Hf][C]
 * (device) = dLoss/dpred -> grad [P] (trainable layout, overwritten; GCN gets none: F2).
 * What loss.backward() computes through HybridSTGCN_LSTM.forward (hybrid_model.py:80-117,
 * train_hybrid_maml_v5.py:134). Consumes the saved activations (ESTATE if there are none). */
int smaml_backward(smaml_ctx* ctx, void* stream, const float* theta, const float* dpred, float* grad);

/* smaml_backward for the most recent smaml_forward, continued through the GCN base: what loss.backward()
 * computes through HybridSTGCN_LSTM.forward when extract_base_features does NOT run under no_grad, i.e. what
 * the reference's freeze_base=False / unfreeze_base_model() promise (hybrid_model.py:16-58,126-134) and its
 * no_grad (F2) withholds. Opt-in: nothing else in the library produces GCN or input gradients.
 *   grad [P]: exactly smaml_backward's result (the same launches; bitwise equal).
 *   gcn_grad (device, optional) [Pg]: the layout of smaml_param_layout(which = 1) (conv{k}.bias, then
 *     conv{k}.lin.weight), overwritten, pads zero: the gradient summed over the samples. 16-byte aligned.
 *   dx_host (optional): dx_host[s] = device pointer to sample s's d loss / d x [T*N][input_channels], 16-byte
 *     aligned. gcn_grad and dx_host both NULL: SMAML_EINVAL (call smaml_backward).
 *   x_host, nsamples: the forward's samples again (the GCN activations are recomputed from them); another
 *     nsamples: SMAML_ESTATE; NULL or misaligned pointers: SMAML_EINVAL. Other states and errors are
 *     smaml_backward's; all are checked before anything is launched, the NULL arguments before a device is needed.
 * After the BPTT, k_lstm_dx0 forms the gradient of the LSTM's layer-0 input from layer 0's gate gradients,
 * dF = dG0 . W_ih0, applies conv4's ReLU derivative from the saved features and writes the per-sample layout
 * (one launch; smaml_set_option("dx0_fused", 0) runs the GEMM + smaml_relu_mask + copies it replaces). conv1..
 * conv3's outputs are then recomputed with the forward's dropout masks (the forward's fused GCN keeps them in
 * registers), and conv4..conv1 run smaml_gcn_conv_backward's launches over all samples (F3: each sample's rows
 * < N aggregate over the graph, the rest see their self loop), the masks replayed on the gradient.
 * Deterministic (fixed-order sums); does not synchronise the stream. Consumes the saved activations like
 * smaml_backward; a smaml_forecast between the forward and this call leaves it valid. The recomputed
 * activations and gradient buffers (nsamples*T*N rows x (3 Hc + 2 max(Hc, Cin) + Cin) floats, plus the GCNConv
 * backward's scratch) are the context's own: they grow only and are freed by smaml_destroy.
 * smaml_adapt_steps_full runs whole steps of one region with this gradient inside the library.
 * smaml_meta_step_base computes the base's meta-gradient inside the meta-step.
 * Not covered: per-task base adaptation in the meta-step's inner loop, p_gcn > 0 there, and
 * smaml_adapt_steps_multi with a trained base. */
int smaml_backward_base(smaml_ctx* ctx, void* stream, const float* theta, const float* const* x_host, int32_t nsamples,
                        const float* dpred, float* grad, float* gcn_grad, float* const* dx_host);

/* In-place train-mode dropout of one STGCN conv output (model.py:33,36,39,42: after conv
 * layer+1's ReLU, STGCN.forward): x [n] (device) gets the counter-based mask of the GCN site
 * `layer` (0..3), seed `seed`, and the 1/(1-p) scale. */
int smaml_dropout(smaml_ctx* ctx, void* stream, float* x, int64_t n, float p, uint32_t seed, int32_t layer);

/* GCN x4 of extract_base_features (hybrid_model.py:60-78, no_grad): x_host[s] = device
 * pointer to sample s's window [T*N][Cin0] -> feats [nsamples][T*N][Hc] (device). */
int smaml_gcn_forward(smaml_ctx* ctx, void* stream, const float* const* x_host, int32_t nsamples, float* feats);

/* nn.LSTM stack (hybrid_model.py:93-102) over layer-0 inputs feats [nsamples][T*N][Hc]
 * (device, row t*N+n) -> hT [nsamples][N][H] (top layer, t = T-1). Saves the activations
 * for smaml_lstm_backward. */
int smaml_lstm_forward(smaml_ctx* ctx, void* stream, const float* theta, const float* feats, int32_t nsamples,
                       float* hT);

/* BPTT after smaml_lstm_forward: dhT [nsamples][N][H] (device) -> the LSTM entries of
 * grad [P] (overwritten; head entries zero). */
int smaml_lstm_backward(smaml_ctx* ctx, void* stream, const float* theta, const float* dhT, float* grad);

/* Head + MSELoss with the F4 row pairing (hybrid_model.py:105-115, train_hybrid_maml_v5.py:
 * 119,133): hT [nsamples][N][H] -> pred [nsamples][N*Hf][C]. With targets (y_host[s] = device
 * pointer to y [Hf*N][C], dataset.py:40-48): loss (1 device float, mean over samples and
 * elements) and dpred = dloss/dpred [nsamples][N*Hf][C]. y_host NULL: prediction only. */
int smaml_head_loss(smaml_ctx* ctx, void* stream, const float* theta, const float* hT, const float* const* y_host,
                    int32_t nsamples, float* pred, float* loss, float* dpred);

/* clip_grad_norm_(max_norm) + SGD(lr) (train_hybrid_maml_v5.py:135-139) on ntasks flat
 * vectors theta/grad [ntasks][P] (device), theta in place; norms [ntasks] (optional). */
int smaml_clip_sgd(smaml_ctx* ctx, void* stream, float* theta, const float* grad, int32_t ntasks, float lr,
                   float max_norm, float* norms);

/* Synchronise `stream` and report device-side failures of this context's kernels: SMAML_EHIP if a
 * grid-barrier bookkeeping kernel (the fused clip + SGD step above, the second-order sweep update)
 * timed out waiting for a grid that was not co-resident (its results are then invalid; the barrier
 * state is reset). Every compute entry point also checks the flag on entry, without syncing.
 * Replaces the implicit error surfacing of torch's synchronous CPU ops at
 * train_hybrid_maml_v5.py:135-139 (`loss.item()` after the inner step). */
int smaml_sync(smaml_ctx* ctx, void* stream);

/* inner_loop_v4 (train_hybrid_maml_v5.py:110-141) for every task of smaml_set_tasks:
 * `steps` support steps of `batch` windows (windows_host [steps+1][ntasks][batch], the last
 * row is the query batch, evaluated but not trained on) -> fast_out [ntasks][P]; losses /
 * norms as in smaml_meta_step. */
int smaml_inner_loop(smaml_ctx* ctx, void* stream, const float* theta, int32_t steps, int32_t batch,
                     const int32_t* windows_host, float inner_lr, float max_norm, float* fast_out, float* losses,
                     float* norms);

/* Device memory on the context's GPU (for hosts without their own allocator). */
int smaml_alloc(smaml_ctx* ctx, int64_t bytes, void** out);
int smaml_free(smaml_ctx* ctx, void* p);

/* ---- RCCL communicator (one process per GPU) ---------------------------- *
 * librccl is loaded on first use. Rank 0 calls smaml_comm_unique_id and ships the 128 bytes
 * to the other ranks (env/file/store); every rank then calls smaml_comm_init. The meta-
 * gradient all-reduce of one meta-step is smaml_comm_allreduce(meta_grad, P) (in-place sum,
 * fp32, on the given stream). The Python path uses torch.distributed's RCCL instead.
 * smaml_comm_init is bounded: where librccl has ncclCommInitRankConfig it creates the
 * communicator non-blocking and polls it for at most smaml_set_option("comm_timeout_ms")
 * (default 120 s); a rank whose peers never arrive gets SMAML_EHIP (communicator aborted)
 * instead of blocking forever, so the ranks can agree on the outcome afterwards. */
int smaml_comm_unique_id(uint8_t* id_out /* 128 bytes */);
int smaml_comm_init(smaml_ctx* ctx, int32_t rank, int32_t world, const uint8_t* id /* 128 bytes */);
int smaml_comm_allreduce(smaml_ctx* ctx, void* stream, float* buf, int64_t n);
int smaml_comm_destroy(smaml_ctx* ctx);

/* ---- measurement (no reference counterpart; bench / profiling only) ------------------ */

/* Enable/disable per-kernel-category HIP-event timing of the launches this context
 * enqueues (events recorded on the launch stream around each kernel). */
int smaml_timing(smaml_ctx* ctx, int32_t enable);

/* Synchronise, then report and reset per category: summed kernel milliseconds, summed
 * algorithmic FLOPs, launch counts (smaml_forecast's launches count under gcn_layer, xg_proj,
 * lstm_fwd_step, head_loss and misc). One kernel symbol per category (index): 0 gcn_layer,
 * 1 lstm_fwd_step, 2 lstm_fwd_dual, 3 head_loss, 4 head_dh, 5 lstm_bwd_step, 6 lstm_bwd_dual,
 * 7 wgrad (split-K GEMM), 8 wgrad_reduce, 9 misc, 10 xg_proj (layer 0's input projection formed before
 * the wavefront: k_xg_dedup once per distinct stream row of consecutive windows, or the batch-1
 * k_gemm_nt), 11 dg_rowsum (k_dg_rowsum: layer 0's dG summed per distinct stream row before its
 * input-weight gradient), 12-15 lstm_fwd_step_wall, lstm_fwd_dual_wall, lstm_bwd_step_wall,
 * lstm_bwd_dual_wall: the wall time of a forward / tangent-forward / BPTT / tangent-BPTT sweep whose
 * diagonals ran as concurrent row chunks on side streams (options fwd_streams / bptt_streams; the
 * per-category kernel times 1, 2, 5, 6 then sum the concurrent chunks' launches). */
int smaml_timing_collect(smaml_ctx* ctx, double* ms, double* flops, int64_t* count, int32_t cap);

/* Launch counts per kernel variant (tile configuration) since the last reset, in the order of
 * kernels.h enum Variant (_capi.VARIANTS): fwd, fwd_drop, fwd_split, fwd_img, fwd_dual,
 * fwd_dual_kept, fwd_dual_img, bwd_big, bwd_small, bwd_split, bwd_dual_big, bwd_dual_big_kept,
 * bwd_dual_small, bwd_dual_small_kept, wgrad, wgrad_wide, wgrad_pair, fwd_kw, bwd_kw, gcn_dedup,
 * xg_dedup, wgrad_dedup, f_compact, gcn_cache (forwards of smaml_meta_step whose GCN features came from the
 * per-stream cache), gcn_cache_rows (stream rows that cache computed: rows, not launches), fwd_infer
 * (smaml_forecast's inference step), fwd_infer_drop (smaml_forecast_ensemble's: one launch per diagonal and
 * member group).
 * Writes min(cap, count) entries, *count = number of variants; reset != 0 zeroes them. Host-side
 * counters: no synchronisation. Lets tests assert which configurations ran. */
int smaml_variant_counts(smaml_ctx* ctx, int64_t* counts, int32_t cap, int32_t* count, int32_t reset);

/* Run-time knobs (tests / A-B; defaults = build-time values):
 *   "bwd_big_min", "bwdd_big_min": primal / tangent BPTT launches with at least this many
 *                                  64-row tile units use the 128x128 tiles (else 64x64 or
 *                                  split-K tiles);
 *   "split_max":                   split-K ways of small-grid LSTM steps (1 = off);
 *   "keep":                        cap on second-order inner steps whose primal is kept
 *                                  (-1 = the SMAML_KEEP environment variable / all that fit);
 *   "wgrad_group_max_rows":        a backward with tasks x rows <= this runs all LSTM weight
 *                                  gradients as one launch after the BPTT (batch-1 adaptation);
 *   "wgrad_group_wgs":             workgroups that grouped launch aims for;
 *   "gcn_fused", "gate_img":       fused GCN stack for the rows t >= 1 / pre-split gate weight
 *                                  images (1 = on, the default);
 *   "wgrad_wide":                  weight gradients whose column count is a multiple of 256 on
 *                                  256 x 256 tiles (1, the default) or 512 x 128 tiles (0);
 *   "wgrad_pair":                  the two passes of a tangent weight gradient (LSTM layers >= 1)
 *                                  as one split-K launch (1, the default) or two (0);
 *   "grid_barrier":                the clip + SGD step and the sweep update as one grid-barrier
 *                                  launch each (1, the default) or two launches each (0; bitwise
 *                                  equal);
 *   "barrier_timeout_us":          bound on a grid-barrier wait (default 4 s); on expiry the kernel
 *                                  exits and the next call / smaml_sync returns SMAML_EHIP;
 *   "comm_timeout_ms":             bound on smaml_comm_init's wait for the other ranks (default
 *                                  120000);
 *   "barrier_oversize":            debug: > 0 launches the grid-barrier kernels with that many
 *                                  times the resident capacity (+1 block), which can never be
 *                                  co-resident, to exercise the bounded wait;
 *   "bwdd_remap":                  tangent BPTT tiles dealt in pair-segment order per XCD (1) or in
 *                                  hardware order (0; bitwise equal);
 *   "small_kw":                    small-grid (batch-1) LSTM forward / BPTT diagonals as one launch
 *                                  with the K reduction split over the waves of a workgroup (1; 2 =
 *                                  also with pre-split BPTT weight images), or as the split-K part +
 *                                  cell launch pair (0);
 *   "adapt_gcn_batch":             smaml_adapt_steps fills its per-window GCN feature cache up front,
 *                                  runs of up to this many consecutive missing windows per GCN pass
 *                                  (default 32; 0 or 1 = one window per step as it is first read;
 *                                  bitwise equal);
 *   "ens_share":                   smaml_forecast_ensemble with p_gcn = 0 runs layer 0 of the LSTM once for
 *                                  all members (default 1; 0 = per member; bitwise equal);
 *   "ens_group":                   smaml_forecast_ensemble runs its members this many at a time (0: all at
 *                                  once; at most 64; -1, the default: the largest group whose rings and
 *                                  per-member features fit 2 GiB; bitwise equal);
 *   "roll_reuse":                  smaml_forecast_rollout computes GCN features and layer 0's projection only
 *                                  for the rows the previous cycle appended (1) or for every row of every
 *                                  window each cycle (0; bitwise equal). Default 1: at config-2 shapes, 32
 *                                  origins x 15 cycles, 44.1 ms (44.0-44.4) against 54.0 ms (53.9-54.1) with 0,
 *                                  outside both spreads (profiles/rollout_bench.log; a Python loop of
 *                                  smaml_forecast calls per cycle: 53.9 ms);
 *   "roll_ens_budget_mb":          smaml_forecast_rollout_ensemble, with ens_group at -1, runs as many members at
 *                                  a time as fit this many MiB of rings, slot tables, sequences and features
 *                                  (at least one; 1 .. 2^20; bitwise equal). Default 32768: at config-2 shapes,
 *                                  32 origins x 15 cycles x 16 members (1.39 GB per member) all 16 at once
 *                                  took 644.7 ms (644.0-645.1) against 651.9 (8 at a time), 664.0 (4) and
 *                                  722.1 ms (721.1-722.4; one at a time, which is what the ensemble's 2 GiB
 *                                  leaves here), each outside the others' spreads
 *                                  (profiles/ensemble_rollout_bench.log). ens_share and roll_reuse apply to this
 *                                  call too: 650.4 ms with ens_share 0, 828.9 ms with roll_reuse 0;
 *   "adapt_group":                 smaml_adapt_steps_multi runs its regions this many at a time, each group
 *                                  as one set of launches per step (0: all at once; at most 64; -1, the
 *                                  default: the measured plan -- 3 to 5 regions in sets of 2, where a set
 *                                  of that size is slower per region than one region alone, every other
 *                                  count all at once);
 *   "dx0_fused":                   smaml_backward_base forms the layer-0 input gradient through conv4's ReLU
 *                                  with k_lstm_dx0 (1, the default) or with the GEMM, ReLU-mask pass and
 *                                  per-sample copies it replaces (0; bitwise equal; measurement only);
 *   "gcn_keep":                    smaml_adapt_steps_full's forward keeps conv1..conv3's outputs for the
 *                                  backward (1, the default) or runs the frozen-base forward and recomputes
 *                                  them per layer as smaml_backward_base does (0; equal within tolerance,
 *                                  not bitwise: the fused and per-layer K orders differ);
 *   "gcn_dz_fused":                smaml_adapt_steps_full forms each layer-to-layer gradient of the base
 *                                  with the GEMM, gather and mask passes over all rows (0, the default) or
 *                                  with k_gcn_dz, one GEMM with the mask in its epilogue plus a gather over
 *                                  the t = 0 rows (1; bitwise equal; measured 0.8 % slower per step at
 *                                  config-4 shapes, so it ships off);
 *   "adapt_phase_sync":            smaml_adapt_steps (and _multi, _full) synchronises its stream after the feature-cache fill
 *                                  and after the step loop so smaml_adapt_phases reports GPU time (0,
 *                                  the default; measurement only);
 *   "gcn_dedup":                   smaml_meta_step steps whose every task reads B consecutive windows
 *                                  run the fused GCN rows t >= 1 once per distinct stream row and
 *                                  store each to every (sample, step) holding it (1, the default;
 *                                  bitwise equal to 0, which computes every sample's rows);
 *   "xg_dedup":                    the same steps form layer 0's input projection F . W_ih0^T (and, in the
 *                                  second-order sweep, F . U_ih0^T) once per distinct stream row
 *                                  (k_xg_dedup) and the big-tile gate kernels start layer 0's
 *                                  accumulators from it (1, the default; the forward adds it in the
 *                                  epilogue: equal to 0 up to f32 rounding, the tangent bitwise);
 *   "wgrad_dedup":                 the same steps form layer 0's input-weight gradient (and its tangent)
 *                                  over the distinct stream rows: dG0 summed per stream row
 *                                  (k_dg_rowsum) times the gathered F rows, (2B + T - 2) N rows
 *                                  instead of T B N (1, the default; equal to 0 up to summation order);
 *   "bptt_streams", "fwd_streams": every BPTT / forward diagonal (primal and tangent) of a large
 *                                  launch split into this many row chunks on side streams (1-4; rows are
 *                                  independent through the whole recurrence, so a chunk's next diagonal
 *                                  fills another's tail; bitwise equal to 1). Defaults: bptt_streams 2,
 *                                  fwd_streams 0 = auto (2 when a problem's gate launch fills at most
 *                                  two workgroups per CU, else 1);
 *   "f_compact":                   where every reader of a step's GCN features goes through the distinct
 *                                  stream rows (xg_dedup forwards on the big tiles, wgrad_dedup
 *                                  backwards), the GCN stores each distinct row once instead of to every
 *                                  (sample, step) holding it (1, the default; bitwise equal to 0).
 *   "gcn_stream_cache":            smaml_meta_step computes the frozen base's features once per stream row
 *                                  and keeps them across inner steps, meta-steps and smaml_set_tasks calls
 *                                  (smaml_gcn_cache_invalidate; 1, the default; bitwise equal to 0);
 *   "gcn_stream_cache_mb":         cap on that cache's bytes in MiB (-1, the default: whatever free HBM
 *                                  allows; 0: no stream gets tables);
 *   "so_f_store":                  0: a second-order meta-step keeps no per-step copy of its GCN features
 *                                  (the sweep asks for them again); 1, the default: best effort, and none
 *                                  where the per-stream cache serves every inner step.
 *   (Round 6 removed the options of arms that measured slower -- bptt_push, wgrad_ws, rowsum_side,
 *   gcn_side, reduce_side, wgrad_overlap, wgrad_min_kt, wgrad_threads, and its own h_img; DESIGN.md
 *   keeps their A/B record.) */
int smaml_set_option(smaml_ctx* ctx, const char* key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* SMAML_H */
