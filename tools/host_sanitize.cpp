// Host-logic checks of libsmaml's C ABI under AddressSanitizer + UBSan (a CPU sanitizer
// build of the host C++). Built by tests/test_host_sanitize_cpu.py from the library's own sources
// (api.cpp with -fsanitize on the host side only, the kernel units host-only), run without a GPU.
// Covers the code that validates and transforms caller input before any launch: dimension checks,
// the parameter layout (state_dict order, 64-float padded offsets), the normalised ELL build of the
// graph (gcn_norm with self loops, in-degree limit), and the error paths of the entry points
// (NULL handles / buffers, no device). Round 5: also the launch-plan builders every kernel launch
// depends on (kernels.h: the LSTM wavefront diagonals, the split-K weight-gradient plans and their
// pairing, the grid-barrier sizing), built with -Werror=missing-field-initializers, each plan checked
// field by field against what was asked for. Also the owning type of every device buffer of the context
// (devbuf.h) over a host allocator: call order, the empty state after a failed grow, the best-effort
// margin, groups. Exit status 0 = every check passed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "devbuf.h"
#include "kernels.h"
#include "smaml.h"

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static smaml_dims dims_cfg2() {
  smaml_dims d;
  d.num_nodes = 441;
  d.window_size = 24;
  d.input_channels = 24;
  d.hidden_channels = 256;
  d.lstm_hidden_size = 128;
  d.lstm_num_layers = 4;
  d.forecast_horizon = 8;
  d.output_channels = 12;
  return d;
}

// 4-neighbour grid graph (both directions), edge_index [2][E]
static std::vector<int64_t> grid_edges(int side) {
  std::vector<int64_t> src, dst;
  for (int r = 0; r < side; ++r)
    for (int c = 0; c < side; ++c) {
      const int i = r * side + c;
      const int nb[4][2] = {{r - 1, c}, {r + 1, c}, {r, c - 1}, {r, c + 1}};
      for (auto& q : nb)
        if (q[0] >= 0 && q[0] < side && q[1] >= 0 && q[1] < side) {
          src.push_back(q[0] * side + q[1]);
          dst.push_back(i);
        }
    }
  std::vector<int64_t> ei(src);
  ei.insert(ei.end(), dst.begin(), dst.end());
  return ei;
}

static smaml::Dims kdims_cfg2() {
  smaml::Dims d;
  d.N = 441;
  d.T = 24;
  d.Cin0 = 24;
  d.Hc = 256;
  d.H = 128;
  d.L = 4;
  d.Hf = 8;
  d.C = 12;
  d.HfC = 96;
  return d;
}

// The wavefront diagonals cover every (layer, step) exactly once, each problem's dependencies lie on
// earlier diagonals, and the block ranges are disjoint, increasing multiples of the per-problem count.
static void check_waves() {
  using namespace smaml;
  const Dims d = kdims_cfg2();
  Work w;
  w.Z = 5;
  w.B = 32;
  w.M = w.B * d.N;
  ParamOff po;
  for (int l = 0; l < d.L; ++l) po.lay[l].cin = l == 0 ? d.Hc : d.H;
  std::set<std::pair<int, int>> fwd, bwd;
  double ffl = 0.0, bfl = 0.0;
  for (int diag = 0; diag < d.T + d.L - 1; ++diag) {
    FwdWave wv;
    ffl += fwd_wave(d, w, po, diag, 16, false, wv);
    CHECK(wv.n >= 1 && wv.n <= d.L && wv.off[0] == 0);
    for (int q = 0; q < wv.n; ++q) {
      CHECK(wv.l[q] + wv.t[q] == diag && wv.l[q] >= 0 && wv.l[q] < d.L && wv.t[q] >= 0 && wv.t[q] < d.T);
      CHECK(wv.off[q + 1] - wv.off[q] == 16);
      CHECK(fwd.insert({wv.l[q], wv.t[q]}).second);
      CHECK(wv.lo[q].cin == po.lay[wv.l[q]].cin);
    }
    BwdWave bv;
    bfl += bwd_wave(d, w, po, diag, 16, false, bv);
    CHECK(bv.n >= 1 && bv.n <= d.L && bv.off[0] == 0);
    for (int q = 0; q < bv.n; ++q) {
      CHECK((d.L - 1 - bv.l[q]) + (d.T - 1 - bv.t[q]) == diag);
      CHECK(bv.off[q + 1] - bv.off[q] == 16);
      CHECK(bwd.insert({bv.l[q], bv.t[q]}).second);
    }
  }
  CHECK((int)fwd.size() == d.L * d.T && (int)bwd.size() == d.L * d.T);
  // LSTM fwd = 2 T N 4H (Hc + H) + 2 T N 4H 2H (L - 1) per sample, less the recurrent
  // products of the t = 0 steps (h_{-1} = 0: not executed, not counted)
  const double lstm = 2.0 * d.T * d.N * 4 * d.H * (d.Hc + d.H) + 2.0 * d.T * d.N * 4 * d.H * 2 * d.H * (d.L - 1) -
                      2.0 * d.N * 4 * d.H * d.H * d.L;
  CHECK(std::fabs(ffl - lstm * w.Z * w.B) <= 1e-9 * ffl);
  CHECK(bfl > 0.0);
}

// plan_wgrad fills every field from its arguments, its K slices cover [0, K) exactly, and its partial
// slabs fit the buffer; pair_wgrad keeps both halves inside the buffer or leaves the plan unchanged.
static void check_wgrad_plans() {
  using namespace smaml;
  Work w;
  w.Z = 5;
  w.B = 32;
  w.M = w.B * 441;
  w.wpart_floats = (int64_t)w.Z * 512 * (256 + 128 + 1) * SMAML_WGRAD_MAXSPLIT;
  w.wpart = reinterpret_cast<float*>(0x1000);
  w.kn.wgrad_wide = 1;
  const float* A = reinterpret_cast<const float*>(0x2000);
  const float* B1 = reinterpret_cast<const float*>(0x3000);
  const float* B2 = reinterpret_cast<const float*>(0x4000);
  float* grad = reinterpret_cast<float*>(0x5000);
  struct Case {
    int Mrows, c1, c2;
    int64_t K;
  } cases[] = {{512, 256, 128, 24LL * 14112}, {512, 128, 128, 24LL * 14112}, {96, 128, 0, 14112},
               {512, 128, 128, 24LL * 441}, {512, 256, 128, 16}, {96, 128, 0, 1}};
  for (const Case& k : cases) {
    WgradPlan p;
    plan_wgrad(w, A, 11, k.Mrows, B1, 12, k.c1, k.c2 ? B2 : nullptr, 13, k.c2, k.K, 7, grad, 606336, 100, 200, 300,
               400, true, false, p);
    CHECK(p.A == A && p.a_zstride == 11 && p.Mrows == k.Mrows && p.B1 == B1 && p.c1 == k.c1 && p.c2 == k.c2);
    CHECK(p.B2 == (k.c2 ? B2 : nullptr) && p.b1_zstride == 12 && p.b2_zstride == 13 && p.K == k.K && p.Mshift == 7);
    CHECK(p.grad == grad && p.P == 606336 && p.off_w1 == 100 && p.off_w2 == 200 && p.off_b1 == 300 && p.off_b2 == 400);
    CHECK(p.with_bias && !p.accumulate && p.Z == w.Z && p.part == w.wpart && p.ldp == k.c1 + k.c2 + 1);
    CHECK(p.ntm >= 1 && p.ntn >= 1 && p.nsplit >= 1 && p.kchunk >= 1);
    CHECK((int64_t)p.nsplit * p.kchunk >= k.K && (int64_t)(p.nsplit - 1) * p.kchunk < k.K);
    CHECK((int64_t)p.nsplit * p.Z * p.Mrows * p.ldp <= w.wpart_floats);
    CHECK(p.A2 == nullptr && p.nsplit1 == 0 && p.drop_layer == -1 && p.drop.thr_lstm == 0);
    WgradPlan q = p;
    if (pair_wgrad(q, w, A, B1, B2)) {
      CHECK(q.nsplit == 2 * q.nsplit1 && q.A2 == A && q.B1s == B1 && q.B2s == B2);
      CHECK((int64_t)q.nsplit1 * q.kchunk >= k.K && (int64_t)(q.nsplit1 - 1) * q.kchunk < k.K);
      CHECK((int64_t)q.nsplit * q.Z * q.Mrows * q.ldp <= w.wpart_floats);
    } else {
      CHECK(q.nsplit == p.nsplit && q.kchunk == p.kchunk && q.A2 == nullptr);
    }
  }
  // a slab buffer too small for two slices: the pair is refused, the plan stays as planned
  Work tiny = w;
  tiny.wpart_floats = (int64_t)w.Z * 512 * 385;
  WgradPlan p;
  plan_wgrad(tiny, A, 0, 512, B1, 0, 256, B2, 0, 128, 24LL * 14112, 0, grad, 0, 0, 0, 0, 0, true, false, p);
  CHECK(p.nsplit == 1);
  CHECK(!pair_wgrad(p, tiny, A, B1, B2) && p.nsplit == 1 && p.A2 == nullptr);
}

static void check_barrier_grid() {
  using smaml::grid_barrier_grid;
  CHECK(grid_barrier_grid(0, 100, 0) == 0);      // capacity unknown: the two-launch form
  CHECK(grid_barrier_grid(1024, 0, 0) == 0);
  CHECK(grid_barrier_grid(1024, 100, 0) == 100);  // fewer items than a quarter of the capacity
  CHECK(grid_barrier_grid(1024, 5000, 0) == 256);
  CHECK(grid_barrier_grid(3, 5000, 0) == 1);
  CHECK(grid_barrier_grid(1024, 5000, 2) == 2049);  // debug oversize: never co-resident
}

// A host allocator for DevBuf (csrc/devbuf.h): malloc / free underneath, the calls logged in order
// ('s' sync, 'f' free, 'a' alloc), a switch that fails the next alloc, a settable free_bytes.
struct FakeAlloc {
  static std::string log;
  static bool fail_next;
  static int64_t room;
  static hipError_t alloc(void** p, int64_t bytes) {
    log += 'a';
    if (fail_next) {
      fail_next = false;
      return hipErrorOutOfMemory;
    }
    *p = std::malloc((size_t)bytes);
    return hipSuccess;
  }
  static hipError_t free(void* p) {
    log += 'f';
    std::free(p);
    return hipSuccess;
  }
  static hipError_t sync() {
    log += 's';
    return hipSuccess;
  }
  static int64_t free_bytes() { return room; }
};
std::string FakeAlloc::log;
bool FakeAlloc::fail_next = false;
int64_t FakeAlloc::room = 0;

// The ownership rule of every device buffer of the context: sync before free, empty after a failure.
static void check_devbuf() {
  using Buf = smaml::DevBuf<FakeAlloc>;
  std::string& log = FakeAlloc::log;
  {
    Buf b;
    CHECK(b.ptr == nullptr && b.cap == 0);
    CHECK(b.grow(100) == hipSuccess && b.ptr && b.cap == 100 && log == "a");  // nothing to free: no sync
    std::memset(b.as<char>(), 1, 100);
    // (a) within capacity: no calls, the same pointer
    void* p = b.ptr;
    log.clear();
    CHECK(b.grow(100) == hipSuccess && b.grow(1) == hipSuccess && b.ptr == p && b.cap == 100 && log.empty());
    // (b) beyond capacity: sync, free, alloc -- no rounding, no minimum
    CHECK(b.grow(101) == hipSuccess && b.cap == 101 && log == "sfa");
    std::memset(b.as<char>(), 2, 101);
    // (c) a failed grow leaves the buffer empty; a smaller grow allocates afresh; release frees nothing
    log.clear();
    FakeAlloc::fail_next = true;
    CHECK(b.grow(1000) == hipErrorOutOfMemory && b.ptr == nullptr && b.cap == 0 && log == "sfa");
    log.clear();
    CHECK(b.release() == hipSuccess && log.empty());
    CHECK(b.grow(50) == hipSuccess && b.ptr && b.cap == 50 && log == "a");
    std::memset(b.as<char>(), 3, 50);
    // (d) grow_if_room: refused at free_bytes <= bytes + margin, a buffer that suffices is kept
    p = b.ptr;
    log.clear();
    FakeAlloc::room = 0;
    CHECK(b.grow_if_room(50, 1 << 20) && b.ptr == p && b.cap == 50 && log.empty());
    FakeAlloc::room = 60 + 10;
    CHECK(!b.grow_if_room(60, 10) && b.ptr == nullptr && b.cap == 0 && log == "sf");  // (not an error: empty)
    FakeAlloc::room = 60 + 10 + 1;
    log.clear();
    CHECK(b.grow_if_room(60, 10) && b.ptr && b.cap == 60 && log == "a");
    FakeAlloc::fail_next = true;
    CHECK(!b.grow_if_room(70, 0) && b.ptr == nullptr && b.cap == 0);  // room, but the allocation fails
    // (e) release twice
    CHECK(b.grow(8) == hipSuccess);
    log.clear();
    CHECK(b.release() == hipSuccess && b.ptr == nullptr && b.cap == 0 && log == "sf");
    CHECK(b.release() == hipSuccess && log == "sf");
    // moved-from buffers own nothing (the kept slots live in a vector); the destructor releases
    CHECK(b.grow(16) == hipSuccess);
    std::vector<Buf> v;
    v.push_back(std::move(b));
    CHECK(b.ptr == nullptr && b.cap == 0 && v[0].cap == 16);
    log.clear();
  }
  CHECK(log == "sf");
  // a group (the graph's five buffers, the four second-order stores): all grown, or all empty
  Buf x, y, z;
  CHECK(smaml::grow_all<FakeAlloc>({{&x, 10}, {&y, 20}, {&z, 30}}) == hipSuccess && x.cap == 10 && y.cap == 20 &&
        z.cap == 30);
  CHECK(smaml::grow_all<FakeAlloc>({{&x, 10}, {&y, 20}, {&z, 30}}) == hipSuccess);
  log.clear();
  FakeAlloc::fail_next = true;
  CHECK(smaml::grow_all<FakeAlloc>({{&x, 5}, {&y, 21}, {&z, 30}}) == hipErrorOutOfMemory);
  CHECK(!x.ptr && !y.ptr && !z.ptr && x.cap == 0 && y.cap == 0 && z.cap == 0 && log == "sfasfsf");
  CHECK(smaml::grow_all<FakeAlloc>({{&x, 5}, {&y, 21}, {&z, 30}}) == hipSuccess && x.cap == 5);
}

int main() {
  CHECK(smaml_abi_version() == 9);
  check_waves();
  check_wgrad_plans();
  check_barrier_grid();
  check_devbuf();
  CHECK(smaml_build_info() != nullptr && std::strlen(smaml_build_info()) > 0);

  // ---- parameter layout (hybrid_model.py state_dict order) ----
  smaml_dims d = dims_cfg2();
  int32_t count = 0;
  int64_t total = 0;
  CHECK(smaml_param_layout(&d, 0, nullptr, nullptr, 0, &count, &total) == 0);
  CHECK(count == 4 * 4 + 2);  // 4 LSTM layers x (W_ih, W_hh, b_ih, b_hh) + head weight, bias
  std::vector<int64_t> off(count), sz(count);
  CHECK(smaml_param_layout(&d, 0, off.data(), sz.data(), count, &count, &total) == 0);
  int64_t nvalid = 0;
  for (int i = 0; i < count; ++i) {
    nvalid += sz[i];
    CHECK(off[i] % 64 == 0);
    if (i) CHECK(off[i] >= off[i - 1] + sz[i - 1]);
  }
  CHECK(nvalid == 606304);  // the 18 trainable tensors
  CHECK(total >= nvalid && total % 64 == 0);
  CHECK(sz[0] == 4 * 128 * 256 && sz[1] == 4 * 128 * 128 && sz[count - 2] == 96 * 128 && sz[count - 1] == 96);
  // a short caller buffer: count and total still reported, only `cap` entries written
  std::vector<int64_t> off2(3, -1);
  CHECK(smaml_param_layout(&d, 0, off2.data(), nullptr, 3, &count, &total) == 0 && count == 18 && off2[2] >= 0);
  CHECK(smaml_param_layout(&d, 1, nullptr, nullptr, 0, &count, &total) == 0 && count == 8);
  CHECK(smaml_param_layout(&d, 2, nullptr, nullptr, 0, &count, &total) == SMAML_EINVAL);
  CHECK(smaml_param_layout(nullptr, 0, nullptr, nullptr, 0, &count, &total) == SMAML_EINVAL);
  smaml_dims bad = d;
  bad.num_nodes = 0;
  CHECK(smaml_param_layout(&bad, 0, nullptr, nullptr, 0, &count, &total) == SMAML_EINVAL);
  bad = d;
  bad.lstm_hidden_size = 100;
  CHECK(smaml_param_layout(&bad, 0, nullptr, nullptr, 0, &count, &total) == SMAML_EINVAL);
  bad = d;
  bad.hidden_channels = 30;
  CHECK(smaml_param_layout(&bad, 0, nullptr, nullptr, 0, &count, &total) == SMAML_EINVAL);
  bad = d;
  bad.lstm_num_layers = 99;
  CHECK(smaml_param_layout(&bad, 0, nullptr, nullptr, 0, &count, &total) == SMAML_EINVAL);
  bad = d;
  bad.output_channels = 48;
  CHECK(smaml_param_layout(&bad, 0, nullptr, nullptr, 0, &count, &total) == SMAML_EINVAL);
  CHECK(std::strlen(smaml_last_error()) > 0);

  // ---- normalised ELL of the graph (PyG gcn_norm: self loops, D^-1/2 (A + I) D^-1/2) ----
  const int side = 21, N = side * side, W = 8;
  std::vector<int64_t> ei = grid_edges(side);
  const int64_t E = (int64_t)ei.size() / 2;
  std::vector<int32_t> cols((size_t)N * W, -1);
  std::vector<float> vals((size_t)N * W, -1.f);
  CHECK(smaml_graph_ell(ei.data(), E, N, cols.data(), vals.data()) == 0);
  std::vector<int> deg(N, 1);
  for (int64_t e = 0; e < E; ++e) deg[ei[E + e]] += 1;
  for (int i = 0; i < N; ++i) {
    bool self = false;
    double wsum = 0.0;
    for (int j = 0; j < W; ++j) {
      const int32_t cidx = cols[(size_t)i * W + j];
      CHECK(cidx >= 0 && cidx < N);
      const float v = vals[(size_t)i * W + j];
      CHECK(std::isfinite(v) && v >= 0.f);
      if (v == 0.f) continue;
      if (cidx == i) {
        self = true;
        CHECK(std::fabs(v - 1.f / deg[i]) < 1e-6f);
      } else {
        CHECK(std::fabs(v - 1.f / std::sqrt((float)deg[i] * (float)deg[cidx])) < 1e-6f);
      }
      wsum += v;
    }
    CHECK(self);
    CHECK(wsum > 0.0);
  }
  // no edges: the self loop alone (weight 1)
  CHECK(smaml_graph_ell(ei.data(), 0, N, cols.data(), vals.data()) == 0);
  CHECK(cols[0] == 0 && vals[0] == 1.f && vals[1] == 0.f);
  // a node id outside [0, N) and an in-degree above the ELL width are rejected
  std::vector<int64_t> badei = {0, 1, 1, N};
  CHECK(smaml_graph_ell(badei.data(), 2, N, cols.data(), vals.data()) == SMAML_EINVAL);
  badei = {-1, 0, 0, 1};
  CHECK(smaml_graph_ell(badei.data(), 2, N, cols.data(), vals.data()) == SMAML_EINVAL);
  std::vector<int64_t> star;  // 8 in-edges into node 0
  for (int k = 1; k <= 8; ++k) star.push_back(k);
  for (int k = 1; k <= 8; ++k) star.push_back(0);
  CHECK(smaml_graph_ell(star.data(), 8, N, cols.data(), vals.data()) == SMAML_EINVAL);
  // an irregular multigraph on 6 nodes, edges in no order: node 0 with 7 in-edges (the edge 1 -> 0 three times), a
  // self loop given once (2) and twice (3), node 5 with no edge at all
  {
    const int n = 6;
    const std::vector<int64_t> s = {4, 1, 3, 2, 1, 3, 2, 1, 3, 4, 0}, t = {0, 0, 3, 0, 0, 0, 2, 0, 3, 0, 1};
    std::vector<int64_t> e2(s);
    e2.insert(e2.end(), t.begin(), t.end());
    std::vector<int32_t> c2((size_t)n * W, -1);
    std::vector<float> v2((size_t)n * W, -1.f);
    CHECK(smaml_graph_ell(e2.data(), (int64_t)s.size(), n, c2.data(), v2.data()) == 0);
    const int want0[W] = {4, 1, 2, 1, 3, 1, 4, 0};  // in input order, then the self loop in the eighth slot
    for (int j = 0; j < W; ++j) CHECK(c2[j] == want0[j] && v2[j] > 0.f);
    CHECK(std::fabs(v2[7] - 1.f / 8.f) < 1e-6f);                      // deg(0) = 7 + 1
    CHECK(std::fabs(v2[1] - 1.f / std::sqrt(8.f * 2.f)) < 1e-6f);      // 1 -> 0: deg(1) = 1 + 1
    for (int i : {2, 3, 5}) {  // input self loops replaced by one; an isolated node keeps it alone
      CHECK(c2[(size_t)i * W] == i && v2[(size_t)i * W] == 1.f);
      for (int j = 1; j < W; ++j) CHECK(c2[(size_t)i * W + j] == i && v2[(size_t)i * W + j] == 0.f);
    }
    std::vector<int64_t> e3(s);  // one more edge into node 0: in-degree 8
    e3.push_back(3);
    e3.insert(e3.end(), t.begin(), t.end());
    e3.push_back(0);
    CHECK(smaml_graph_ell(e3.data(), (int64_t)s.size() + 1, n, c2.data(), v2.data()) == SMAML_EINVAL);
    CHECK(std::strstr(smaml_last_error(), "in-degree") != nullptr);
    const std::vector<int64_t> negt = {0, 1, 1, -1};  // a negative target
    CHECK(smaml_graph_ell(negt.data(), 2, n, c2.data(), v2.data()) == SMAML_EINVAL);
    const std::vector<int64_t> loop7 = {7, 1, 7, 2};  // a self loop outside the graph
    CHECK(smaml_graph_ell(loop7.data(), 2, n, c2.data(), v2.data()) == SMAML_EINVAL);
  }
  CHECK(smaml_graph_ell(nullptr, 2, N, cols.data(), vals.data()) == SMAML_EINVAL);
  CHECK(smaml_graph_ell(ei.data(), E, 0, cols.data(), vals.data()) == SMAML_EINVAL);

  // ---- the same adjacency as CSR (smaml_graph_csr: any in-degree, optional weights) ----
  {
    // the grid graph: the CSR rows are the ELL's non-zero entries, in order, bit for bit
    std::vector<int32_t> rp((size_t)N + 1, -1), cc((size_t)E + N, -1);
    std::vector<float> cv((size_t)E + N, -1.f);
    int64_t nnz = -1;
    CHECK(smaml_graph_ell(ei.data(), E, N, cols.data(), vals.data()) == 0);
    CHECK(smaml_graph_csr(ei.data(), nullptr, E, N, rp.data(), cc.data(), cv.data(), E + N, &nnz) == 0);
    CHECK(nnz == E + N && rp[0] == 0 && rp[N] == nnz);
    for (int i = 0; i < N; ++i) {
      int32_t e = rp[i];
      for (int j = 0; j < W; ++j) {
        if (vals[(size_t)i * W + j] == 0.f) continue;
        CHECK(e < rp[i + 1] && cc[e] == cols[(size_t)i * W + j] &&
              std::memcmp(&cv[e], &vals[(size_t)i * W + j], sizeof(float)) == 0);
        ++e;
      }
      CHECK(e == rp[i + 1]);
    }
    // the star the ELL rejects, weighted; a zero weight, a weighted self loop given twice (the last one stays)
    std::vector<int64_t> st;
    for (int k = 1; k <= 8; ++k) st.push_back(k);
    st.insert(st.end(), {0, 0});
    for (int k = 1; k <= 8; ++k) st.push_back(0);
    st.insert(st.end(), {0, 0});
    std::vector<float> sw = {1.f, 2.f, 0.f, 4.f, 0.5f, 1.f, 1.f, 1.f, 0.25f, 3.f};
    const int n = 9;
    std::vector<int32_t> rp9((size_t)n + 1, -1);
    CHECK(smaml_graph_csr(st.data(), sw.data(), 10, n, rp9.data(), cc.data(), cv.data(), 5, &nnz) == SMAML_EINVAL);
    CHECK(nnz == 7 + n && rp9[0] == -1 && std::strstr(smaml_last_error(), "cap") != nullptr);  // nnz written, rowptr not
    CHECK(smaml_graph_csr(st.data(), sw.data(), 10, n, rp9.data(), cc.data(), cv.data(), 16, &nnz) == 0);
    CHECK(nnz == 16 && rp9[1] == 8 && cc[7] == 0);                          // 7 in-edges (the zero one dropped) + loop
    const float deg0 = 3.f + 1.f + 2.f + 4.f + 0.5f + 1.f + 1.f + 1.f;      // loop 3 (the last) + the weights
    CHECK(std::fabs(cv[7] - 3.f / deg0) < 1e-6f);
    CHECK(cc[0] == 1 && cc[2] == 4 && std::fabs(cv[2] - 4.f / std::sqrt(deg0 * 1.f)) < 1e-6f);
    double row0 = 0.0;
    for (int e = rp9[0]; e < rp9[1]; ++e) row0 += cv[e];
    CHECK(row0 > 0.0);
    // rejections name the edge; *nnz_out is still written
    for (float bad : {-1.f, NAN, INFINITY}) {
      sw[4] = bad;
      nnz = -1;
      CHECK(smaml_graph_csr(st.data(), sw.data(), 10, n, rp9.data(), cc.data(), cv.data(), 16, &nnz) == SMAML_EINVAL);
      CHECK(nnz == 0 && std::strstr(smaml_last_error(), "edge 4") != nullptr);
    }
    std::vector<int64_t> badcsr = {0, 1, 1, n};
    CHECK(smaml_graph_csr(badcsr.data(), nullptr, 2, n, rp9.data(), cc.data(), cv.data(), 16, &nnz) == SMAML_EINVAL);
    CHECK(std::strstr(smaml_last_error(), "edge 1") != nullptr);
    badcsr = {-1, 0, 0, 1};
    CHECK(smaml_graph_csr(badcsr.data(), nullptr, 2, n, rp9.data(), cc.data(), cv.data(), 16, &nnz) == SMAML_EINVAL);
    CHECK(smaml_graph_csr(nullptr, nullptr, 2, n, rp9.data(), cc.data(), cv.data(), 16, &nnz) == SMAML_EINVAL);
    CHECK(smaml_graph_csr(st.data(), nullptr, 10, n, rp9.data(), cc.data(), cv.data(), 16, nullptr) == SMAML_EINVAL);
    // no edges: every row its loop of weight 1
    CHECK(smaml_graph_csr(st.data(), nullptr, 0, n, rp9.data(), cc.data(), cv.data(), 16, &nnz) == 0);
    CHECK(nnz == n && rp9[n] == n && cc[n - 1] == n - 1 && cv[0] == 1.f);
    CHECK(smaml_set_graph_weighted(nullptr, st.data(), nullptr, 10) == SMAML_EINVAL);
    int64_t gst[5];
    CHECK(smaml_graph_stats(nullptr, gst, 5, nullptr) == SMAML_EINVAL);
  }

  // ---- entry points on a NULL handle / without a device ----
  smaml_ctx* ctx = nullptr;
  const int rc = smaml_create(&d, 0, &ctx);
  if (rc == 0) {  // a device is present: the handle must be usable and destroyable
    CHECK(ctx != nullptr);
    CHECK(smaml_set_option(ctx, "no_such_knob", 1) == SMAML_EINVAL);
    CHECK(smaml_set_option(ctx, "keep", -2) == SMAML_EINVAL);
    CHECK(smaml_set_dropout(ctx, 1.5f, 0.f, 0) == SMAML_EINVAL);
    // a refused graph and a refused reservation leave a context that destroys cleanly
    CHECK(smaml_set_graph(ctx, badei.data(), 2) == SMAML_EINVAL);
    CHECK(smaml_reserve(ctx, 1, 1 << 20) == SMAML_EINVAL);
    CHECK(smaml_destroy(ctx) == 0);
  } else {
    CHECK(ctx == nullptr);
    CHECK(rc == SMAML_EINVAL || rc == SMAML_EHIP);
  }
  CHECK(smaml_create(&d, -1, &ctx) != 0);
  CHECK(smaml_create(&bad, 0, &ctx) == SMAML_EINVAL);
  CHECK(smaml_create(&d, 0, nullptr) == SMAML_EINVAL);
  CHECK(smaml_destroy(nullptr) == 0);
  int32_t ids[2] = {0, 1};
  CHECK(smaml_set_task_ids(nullptr, ids, 2) == SMAML_EINVAL);
  CHECK(smaml_set_dropout(nullptr, 0.1f, 0.1f, 1) == SMAML_EINVAL);
  CHECK(smaml_set_option(nullptr, "keep", 1) == SMAML_EINVAL);
  CHECK(smaml_sync(nullptr, nullptr) == SMAML_EINVAL);
  CHECK(smaml_set_option(nullptr, "barrier_timeout_us", 1000) == SMAML_EINVAL);
  CHECK(smaml_meta_step(nullptr, nullptr, nullptr, 2, 1, 1, nullptr, 0.01f, 1.f, 0.5f, nullptr, nullptr, nullptr,
                        nullptr) == SMAML_EINVAL);
  // smaml_forecast's argument checks (nothing launches): no output asked for, no windows, no context
  {
    const int32_t win[2] = {0, 1};
    float* some_pred = reinterpret_cast<float*>(0x1000);   // never dereferenced: every call fails before
    double* some_skill = reinterpret_cast<double*>(0x2000);
    const float* some_theta = reinterpret_cast<const float*>(0x3000);
    CHECK(smaml_forecast(nullptr, nullptr, some_theta, 0, win, 2, 2, nullptr, nullptr, nullptr) == SMAML_EINVAL);
    CHECK(std::strstr(smaml_last_error(), "both NULL") != nullptr);
    CHECK(smaml_forecast(nullptr, nullptr, some_theta, 0, win, 0, 2, nullptr, some_pred, nullptr) == SMAML_EINVAL);
    CHECK(std::strstr(smaml_last_error(), "nwin") != nullptr);
    CHECK(smaml_forecast(nullptr, nullptr, some_theta, 0, win, -3, 2, nullptr, nullptr, some_skill) == SMAML_EINVAL);
    CHECK(smaml_forecast(nullptr, nullptr, some_theta, 0, win, 2, 0, nullptr, some_pred, nullptr) == SMAML_EINVAL);
    CHECK(smaml_forecast(nullptr, nullptr, some_theta, 0, nullptr, 2, 2, nullptr, some_pred, nullptr) == SMAML_EINVAL);
    CHECK(smaml_forecast(nullptr, nullptr, some_theta, 0, win, 2, 2, nullptr, some_pred, some_skill) == SMAML_EINVAL);
    CHECK(std::strstr(smaml_last_error(), "ctx is NULL") != nullptr);
    CHECK(smaml_forecast_bytes(nullptr) == 0);
  }
  // smaml_backward_base's argument checks (nothing launches): no output asked for, NULL inputs, no context
  {
    float* some = reinterpret_cast<float*>(0x1000);  // never dereferenced: every call fails before
    const float* xs[1] = {some};
    float* dxs[1] = {some};
    CHECK(smaml_backward_base(nullptr, nullptr, some, xs, 1, some, some, nullptr, nullptr) == SMAML_EINVAL);
    CHECK(std::strstr(smaml_last_error(), "both NULL") != nullptr);
    CHECK(smaml_backward_base(nullptr, nullptr, nullptr, xs, 1, some, some, some, dxs) == SMAML_EINVAL);
    CHECK(smaml_backward_base(nullptr, nullptr, some, nullptr, 1, some, some, some, dxs) == SMAML_EINVAL);
    CHECK(smaml_backward_base(nullptr, nullptr, some, xs, 0, some, some, some, dxs) == SMAML_EINVAL);
    CHECK(smaml_backward_base(nullptr, nullptr, some, xs, 1, nullptr, some, some, dxs) == SMAML_EINVAL);
    CHECK(smaml_backward_base(nullptr, nullptr, some, xs, 1, some, nullptr, some, dxs) == SMAML_EINVAL);
    CHECK(std::strstr(smaml_last_error(), "bad backward_base arguments") != nullptr);
    CHECK(smaml_backward_base(nullptr, nullptr, some, xs, 1, some, some, some, nullptr) == SMAML_EINVAL);
    CHECK(std::strstr(smaml_last_error(), "ctx is NULL") != nullptr);
  }
  CHECK(smaml_reserve(nullptr, 1, 1) == SMAML_EINVAL);
  CHECK(smaml_set_graph(nullptr, ei.data(), E) == SMAML_EINVAL);
  CHECK(smaml_variant_counts(nullptr, nullptr, 0, nullptr, 0) == SMAML_EINVAL);
  CHECK(smaml_workspace_bytes(nullptr) == 0 && smaml_so_kept_steps(nullptr) == 0);

  if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
  else std::printf("host sanitize checks: all passed\n");
  return failures ? 1 : 0;
}
