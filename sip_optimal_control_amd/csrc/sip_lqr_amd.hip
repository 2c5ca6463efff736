// sip_lqr_amd.hip -- C ABI (include/sip_lqr_amd.h) over the gfx950 kernels.
// Host side of the drop-in boundary; no CPU compute path exists here.
#include "../../include/sip_lqr_amd.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <new>
#include <optional>
#include <vector>

#include "chain_embed.hpp"
#include "chain_mf32.hpp"
#include "mt16_launch.hpp"
#include "qf32_launch.hpp"
#include "generic_plan.hpp"
#include "qw16_table.hpp"
#include "residual_launch.hpp"
#include "stream_fill.hpp"
#include "vjp_cols_launch.hpp"
#include "vjp_launch.hpp"

using sipamd::KernelEntry;

// Where the regions of a plan's one workspace buffer start, in bytes.  It serves the fused kernel (+ the scratch of
// its split entry points and of the embedding) and the general engine, never both at once: `total` is the larger.
struct Workspace {
  // fused kernel: spill (at 0) | scratch vecs (zero rhs of factor) | scratch sol | status copy (for sip_lqr_solve,
  // which has no status argument) | G factors of the split factor | embedded mats | embedded gains
  size_t vecs = 0, sol = 0, status = 0, gfac = 0, pmats = 0, pgains = 0;
  // general engine: work arena (at 0) | status copy
  size_t general_status = 0;
  size_t total = 0;
};

// A plan is its shape, the kernel row that serves it and what follows from the two (decide_kernel).
struct sip_lqr_plan {
  int layout = SIP_LQR_LAYOUT_FULL; // of mats
  int dtype = SIP_LQR_F64;
  int64_t batch = 0;
  int T = 0, n = 0, m = 0, device = 0;
  // the dedicated kernel of the plan; nullptr: the general engine (tree_generic.hpp) runs factor then solve
  const KernelEntry *kernel = nullptr;
  const char *kernel_name = "";
  // General engine on the packed chain layout: serves shapes / dtypes without
  // a dedicated kernel and the split factor / solve entry points.  Tables are
  // laid out and uploaded at plan creation, so that the compute entry points
  // only enqueue kernels (graph-capturable from the first call on).
  sipamd::GenericPlan gen;
  // false: the plan was created on a host without a HIP device and serves the
  // host-side entry points only (sizes, pack / unpack, kernel name).
  bool on_device = false;
  // Split factor / solve of a shape with a fused kernel: both re-run the fused sweep (factor on a
  // zero right-hand side), which beats a second, slower kernel family by an order of magnitude;
  // SIP_LQR_SPLIT=general keeps them on the general engine.
  bool split_on_fused = false;
  // Uniform shapes without an exact kernel run on the next larger fused kernel (dims.N >= n, dims.M >= m) through the
  // embedding of chain_embed.hpp.  SIP_LQR_PAD=0 keeps the general engine.  Not padded: dims.N = n, dims.M = m.
  bool padded = false;
  sipamd::embed::PadDims dims{};
  // sip_lqr_plan_set_separate_sweeps on a plan whose kernel row has them: factor and solve as sweeps of their own
  // (chain_factor_mt16, chain_solve_mt16; chain_factor_qf32, chain_solve_cols_qf32 on a plan with fused_f32)
  bool separate = false;
  // sip_lqr_plan_set_fused_f32 on an fp32 plan of the general engine whose shape has a row in kQf32Rows: the plan
  // runs on chain_factor_solve_qf32.  forced_general: SIP_LQR_VARIANT=general at creation, which the opt-in respects
  bool fused_f32 = false;
  bool forced_general = false;
  // sip_lqr_plan_set_wide_controls on a FULL-layout plan of the general engine with 9 <= m <= 16, n <= 32: the plan
  // runs on a row of kWideRows, its own (n = 32, m in {12, 16}) or, in fp64, embedded in the one with the least M >= m
  bool wide_controls = false;
  // sip_lqr_factor_solve runs on the row's launch_park: the fused sweep that keeps the spill slots of its first nodes
  // in accumulation registers (chain_qw16.hpp, PARK), so that the workspace holds no complete factor state after it.
  // The plan's own shape only (not through the embedding), unless SIP_LQR_PARK=0 at creation; sip_lqr_kernel_name
  // then ends in ",park".  Every other sweep of the plan is the row's launch_fs, launch_mrhs or launch_split.
  bool park = false;
  std::string name_storage;
  Workspace ws;

  // a solve that reads only the vectors against the state a factor call left: mode 2 of the kernel, or its solve sweep
  bool has_solve_mode() const { return separate || (kernel != nullptr && kernel->solve_only); }
  // the fused sweep with A | B read in place: for the plan's own shape only, not through the embedding
  sipamd::launch_split_t launch_split() const { return kernel != nullptr && !padded ? kernel->launch_split : nullptr; }
};

// Overridden by the object __graft_entry__.build_hip() generates (build_stamp.c); a library linked
// without it (tools/diag_build.sh) says so.
extern "C" __attribute__((weak)) const char sip_lqr_build_stamp[] = "SIPLQRSRC=unstamped";

#ifdef SIP_LQR_STAMPS
// Diagnostic build: device buffer of 8 x u64 per wave, set by the tool.
unsigned long long *g_sip_lqr_stamps = nullptr;
extern "C" void sip_lqr_debug_set_stamps(void *p) { g_sip_lqr_stamps = (unsigned long long *)p; }
#endif

namespace {

using sipamd::report;

template <int M>
hipError_t launch_mf32(long batch, int T, const void *mats, const void *vecs, void *sol, void *gains,
                       int32_t *status, void *ws, hipStream_t stream, int /*mode: always the full sweep*/,
                       void * /*gfac*/) {
  hipLaunchKernelGGL((sipamd::mf32::chain_factor_solve_mf32<M>), dim3((unsigned)batch), dim3(64), 0,
                     stream, (const float *)mats, (const float *)vecs, (float *)sol, (float *)gains,
                     (float *)ws, (int *)status, batch, T SIP_STAMP_PASS);
  return hipGetLastError();
}

// fp32, n = 32: one problem per wavefront, products on the matrix cores
#define MF32(M)                                                                \
  { SIP_LQR_F32, 32, M, "chain_factor_solve_mf32<32," #M ",mfma>/f32",          \
    sipamd::mf32::Layout<M>::WSN, &launch_mf32<M> }

// n = 32 on 16 x 16 matrix-core tiles (chain_mt16.hpp), fp32 and fp64; the 32x32x2 kernel of round 1
// (chain_mf32.hpp) stays selectable by SIP_LQR_VARIANT=mf32 for A/B timing
const KernelEntry kKernels[] = {
    MT16_ENTRY(SIP_LQR_F32, float, "f32", 8),  MT16_ENTRY(SIP_LQR_F32, float, "f32", 4),
    MT16_ENTRY(SIP_LQR_F64, double, "f64", 8), MT16_ENTRY(SIP_LQR_F64, double, "f64", 4),
    MF32(8),
};

// fp32, n <= 15: four problems per wavefront on v_fmac_f32_dpp (chain_qf32.hpp).  A table of its own that find_kernel
// never searches: a plan gets one of these rows through sip_lqr_plan_set_fused_f32 alone.
const KernelEntry kQf32Rows[] = {SIP_QF32_ROWS(QF32_ENTRY)};

// n = 32 on 16 x 16 matrix-core tiles with 12 and 16 controls (chain_mt16_wide.hip, chain_mt16_wide_solve.hip), by
// ascending M per dtype.  A table of its own that find_kernel and find_embedding_kernel never search: a plan gets one of
// these rows through sip_lqr_plan_set_wide_controls alone.
const KernelEntry kWideRows[] = {
    MT16_ENTRY(SIP_LQR_F32, float, "f32", 12),  MT16_ENTRY(SIP_LQR_F32, float, "f32", 16),
    MT16_ENTRY(SIP_LQR_F64, double, "f64", 12), MT16_ENTRY(SIP_LQR_F64, double, "f64", 16),
};

// The dispatch environment, read whenever a plan is created or opted in (tests change it between plans).
struct DispatchEnv {
  const char *variant;  // SIP_LQR_VARIANT (tests, A/B timing): only kernels whose name carries the tag; nullptr: any
  bool general;         // SIP_LQR_VARIANT=general: no dedicated kernel at all
  bool core_only;       // SIP_LQR_EXTRA=0 (tests of the embedding): hides the slice entries outside the core set
  bool pad;             // SIP_LQR_PAD=0 clears it: no embedding
  bool split_general;   // SIP_LQR_SPLIT=general: split factor / solve stay on the general engine
  int park;             // SIP_LQR_PARK (A/B timing, the bitwise test), where the plan's row has a parked fused sweep
                        // (KernelEntry::launch_park): 0 keeps the plain kernel, 1 takes the parked one at any batch;
                        // unset (-1): the parked one from park_min_batch() of the plan's device on
};
// The parked sweep trades HBM bytes for instructions on the wavefront's critical path: it wins where the launch is
// bound by the memory side (batch 4096, four wavefronts per CU: -5 %) and loses where one wavefront per CU runs at its
// own latency (batch 1024: +5 %).  In between the two layouts go either way by 1-3 %, so the
// default parks where the win is measured: from four wavefronts per CU on -- LDS holds no more, so from there on
// every SIMD of the chip runs one -- at four problems per wavefront: 16 problems per CU, batch 4096 on the 256 CUs
// of an MI355X.  A plan without a device (host-side entry points only) does not park.
int64_t park_min_batch(int device) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    return INT64_MAX;
  }
  return 16 * (int64_t)cus;
}
DispatchEnv dispatch_env() {
  auto is = [](const char *key, const char *value) {
    const char *v = std::getenv(key);
    return v != nullptr && std::strcmp(v, value) == 0;
  };
  const char *variant = std::getenv("SIP_LQR_VARIANT"), *extra = std::getenv("SIP_LQR_EXTRA");
  if (variant != nullptr && variant[0] == 0)
    variant = nullptr;
  return {variant, is("SIP_LQR_VARIANT", "general"), extra != nullptr && extra[0] == '0', !is("SIP_LQR_PAD", "0"),
          is("SIP_LQR_SPLIT", "general"), is("SIP_LQR_PARK", "0") ? 0 : is("SIP_LQR_PARK", "1") ? 1 : -1};
}

// kKernels, then the fused fp64 kernels of every shape n <= 16, m <= 8 (the slices of qw16_kernels.hip, where
// the alternatives of a shape stand together, the default first).
template <typename F> void for_each_kernel(const DispatchEnv &env, F &&f) {
  for (const auto &k : kKernels)
    f(k);
  typedef const KernelEntry *(*slice_fn)(int *);
#define SIP_QW16_SLICE_FN(S) sipamd::qw16_slice_##S,
  static const slice_fn slices[QW16_SLICE_COUNT] = {QW16_FOR_EACH_SLICE(SIP_QW16_SLICE_FN)};
#undef SIP_QW16_SLICE_FN
  for (const slice_fn fn : slices) {
    int count = 0;
    const KernelEntry *table = fn(&count);
    for (int e = 0; e < count; ++e)
      if (table[e].core || !env.core_only)
        f(table[e]);
  }
}

// First match wins.
const KernelEntry *find_kernel(const DispatchEnv &env, int dtype, int n, int m, int layout) {
  const KernelEntry *found = nullptr;
  for_each_kernel(env, [&](const KernelEntry &k) {
    if (found == nullptr && k.dtype == dtype && k.n == n && k.m == m && k.layout == layout &&
        (env.variant == nullptr || std::strstr(k.name, env.variant)))
      found = &k;
  });
  return found;
}

// Smallest fused fp64 kernel that can embed an (n, m) chain: least N, then a staged kernel with
// the least M, then a direct one.  Called when no visible kernel has the shape itself: what can still hold
// it is in kKernels or, with SIP_LQR_EXTRA=0, the core set.
const KernelEntry *find_embedding_kernel(const DispatchEnv &env, int n, int m) {
  const KernelEntry *best = nullptr;
  auto better = [&](const KernelEntry &k) {
    if (best == nullptr)
      return true;
    if (k.n != best->n)
      return k.n < best->n;
    if (k.staged != best->staged)
      return k.staged;
    return k.m < best->m;
  };
  for_each_kernel(env, [&](const KernelEntry &k) {
    if (k.dtype == SIP_LQR_F64 && k.layout == SIP_LQR_LAYOUT_FULL && k.n >= n && k.m >= m && better(k))
      best = &k;
  });
  return best;
}

size_t scalar_size(const sip_lqr_plan *p) {
  return p->dtype == SIP_LQR_F32 ? sizeof(float) : sizeof(double);
}
sipamd::ChainLens lens(const sip_lqr_plan *p) { return sipamd::chain_lens(p->n, p->m, p->T, p->layout); }

// Chain topology (Topology::set_chain, lqr.cpp:32-40) for the general engine.
void init_generic(sip_lqr_plan *p) {
  const int T = p->T, N = T + 1;
  std::vector<int> sd(N, p->n), cd(T, p->m), pa(T), ch(T);
  for (int e = 0; e < T; ++e)
    pa[e] = e, ch[e] = e + 1;
  sipamd::GenericPlan &g = p->gen;
  g.set_shape(T, 0, sd.data(), cd.data());
  (void)g.compile(pa.data(), ch.data());
  g.layout_chain(p->n, p->m, T);
}

Workspace workspace_layout(const sip_lqr_plan *p) {
  const size_t B = (size_t)p->batch, T = p->T, M = p->dims.M, bytes = B * scalar_size(p);
  const sipamd::ChainLens host = sipamd::chain_lens(p->dims.N, p->dims.M, p->T, SIP_LQR_LAYOUT_FULL);
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const bool scratch = p->split_on_fused || p->padded;
  Workspace w;
  w.vecs = up(bytes * (T + 1) * (size_t)(p->kernel ? p->kernel->ws_slot : 0));
  w.sol = w.vecs + (scratch ? up(bytes * host.vecs) : 0); // vecs / sol in the kernel's dimensions
  w.status = w.sol + (scratch ? up(bytes * host.vecs) : 0);
  w.gfac = w.status + (scratch ? up(B * sizeof(int32_t)) : 0);
  w.pmats = w.gfac + (p->split_on_fused ? up(bytes * T * (M * M + M)) : 0);
  w.pgains = w.pmats + (p->padded ? up(bytes * host.mats) : 0);
  const size_t fused_total = w.pgains + (p->padded ? up(bytes * host.gains) : 0);
  w.general_status = (bytes * (size_t)p->gen.ws_len + 15) / 16 * 16;
  w.total = std::max(fused_total, w.general_status + B * sizeof(int32_t));
  return w;
}

// Point the plan at its kernel row (nullptr: the general engine; embedded: a row of a larger shape) and recompute
// what follows from it.  At creation and again by the fp32 and the wide-controls opt-ins, after init_generic.
void decide_kernel(sip_lqr_plan *p, const KernelEntry *k, bool embedded, const DispatchEnv &env) {
  p->kernel = k;
  p->padded = embedded;
  p->dims = sipamd::embed::pad_dims(p->n, p->m, embedded ? k->n : p->n, embedded ? k->m : p->m, p->T);
  p->park = k != nullptr && !embedded && k->launch_park != nullptr &&
            (env.park == 1 || (env.park < 0 && p->batch >= park_min_batch(p->device)));
  if (embedded)
    p->name_storage = std::string(k->name) + " embedding (" + std::to_string(p->n) + "," + std::to_string(p->m) + ")";
  else if (p->park)
    p->name_storage = std::string(k->name) + ",park";
  p->kernel_name = embedded || p->park ? p->name_storage.c_str()
                   : k      ? k->name
                            : (p->dtype == SIP_LQR_F32 ? "tree_generic(chain layout)/f32"
                                                       : "tree_generic(chain layout)/f64");
  p->split_on_fused = k != nullptr && (p->layout != SIP_LQR_LAYOUT_FULL || !env.split_general);
  p->ws = workspace_layout(p);
}

// How sip_lqr_solve_multi carries `num_rhs` columns: launch == nullptr: column by column through sip_lqr_solve, no
// column workspace; else `columns` per launch and `scalars` of column workspace per problem.
struct ColumnSweep {
  sipamd::launch_cols_t launch = nullptr;
  int columns = 0;
  long scalars = 0;
};
ColumnSweep column_sweep(const sip_lqr_plan *p, int num_rhs) {
  if (p->kernel == nullptr || p->padded || !p->split_on_fused)
    return {};
  if (p->separate) { // the solve sweep of the row: what it keeps per node and column is the row's to say
    const KernelEntry &k = *p->kernel;
    return {k.launch_solve_sweep, k.sweep_columns,
            (long)(p->T + 1) * std::min(num_rhs, k.sweep_columns) * k.sweep_col_scalars};
  }
  if (p->kernel->launch_mrhs != nullptr) // chain_mrhs.hpp: g | h | k per node and column
    return {p->kernel->launch_mrhs, sipamd::kMrhsColumns,
            (long)(p->T + 1) * std::min(num_rhs, sipamd::kMrhsColumns) * (2 * p->n + p->m)};
  return {};
}

// The preamble of every compute entry point: the plan must live on a device (see sip_lqr_plan::on_device), which is
// the current one while this lives.  rc != SIP_LQR_OK: reported under the entry point's name, to be returned.
struct OnPlanDevice {
  std::optional<sipamd::DeviceGuard> guard;
  int rc;
  OnPlanDevice(const sip_lqr_plan *p, const char *what) {
    if (!p->on_device) {
      rc = report(hipErrorNoDevice, what);
      return;
    }
    guard.emplace(p->device);
    rc = guard->err == hipSuccess ? SIP_LQR_OK : report(guard->err, (std::string(what) + "(hipSetDevice)").c_str());
  }
};

// The general engine's two launches, by the plan's dtype.
hipError_t general_factor(const sip_lqr_plan *p, const void *mats, void *ws, void *gains, int32_t *status,
                          hipStream_t s) {
  return p->dtype == SIP_LQR_F32 ? p->gen.launch_factor<float>(p->batch, mats, ws, gains, status, s)
                                 : p->gen.launch_factor<double>(p->batch, mats, ws, gains, status, s);
}
hipError_t general_solve(const sip_lqr_plan *p, const void *mats, const void *vecs, void *ws, void *gains, void *sol,
                         const int32_t *status, hipStream_t s) {
  return p->dtype == SIP_LQR_F32 ? p->gen.launch_solve<float>(p->batch, mats, vecs, ws, gains, sol, status, s)
                                 : p->gen.launch_solve<double>(p->batch, mats, vecs, ws, gains, sol, status, s);
}

// What a sweep of the plan's kernel does; the values are the `mode` of launch_fs_t.
enum class Sweep : int {
  Full = 0,   // fused factor + solve
  Factor = 1, // split factor (vecs == nullptr: zero right-hand side; sol not wanted)
  Solve = 2,  // split solve against the state a Factor call left in `ws` (and, unpadded, in `gains`): only for a plan
              // that has_solve_mode(), the others ask for Full again
};

// The sweep of a plan, through the embedding when the plan is padded.  A plan with the separate sweeps runs its factor
// sweep for Factor and its solve sweep (one column; g and k through the spill and the gains) for Solve.
hipError_t run_fused(const sip_lqr_plan *p, const void *mats, const void *vecs, void *sol, void *gains,
                     int32_t *status, void *ws, hipStream_t s, Sweep mode) {
  const Workspace &f = p->ws;
  const KernelEntry &k = *p->kernel;
  const long B = p->batch;
  char *w = (char *)ws;
  const bool factor_sweep = p->separate && mode == Sweep::Factor; // reads no right-hand side
  const bool solve_sweep = p->separate && mode == Sweep::Solve;   // writes nothing for a problem whose factor failed
  // the buffers the sweep sees: the caller's, or the embedding's regions of the workspace
  const void *km = p->padded ? w + f.pmats : mats, *kv = p->padded || vecs == nullptr ? w + f.vecs : vecs;
  void *ksol = p->padded || sol == nullptr ? w + f.sol : sol, *kgains = p->padded ? w + f.pgains : gains;
  hipError_t e = hipSuccess;
  if (p->padded) // the padded matrices (and gains) of the factor call are still in the workspace for Solve
    sipamd::embed::embed_inputs(p->dims, B, mode != Sweep::Solve ? mats : nullptr, w + f.pmats, vecs, w + f.vecs, s);
  if (vecs == nullptr && !factor_sweep)
    e = sipamd::zero_async(w + f.vecs, f.sol - f.vecs, s);
  if (e == hipSuccess)
    e = factor_sweep  ? k.launch_factor_sweep(B, p->T, km, kgains, status, ws, w + f.gfac, s)
        : solve_sweep ? k.launch_solve_sweep(B, p->T, km, kv, ksol, kgains, ws, w + f.gfac, nullptr, status, 1, 0L, s)
        : p->park && mode == Sweep::Full ? k.launch_park(B, p->T, km, kv, ksol, kgains, status, ws, s, 0, w + f.gfac)
                      : k.launch_fs(B, p->T, km, kv, ksol, kgains, status, ws, s, (int)mode, w + f.gfac);
  if (e == hipSuccess && p->padded)
    sipamd::embed::extract_outputs(p->dims, B, w + f.sol, sol, solve_sweep ? status : nullptr, w + f.pgains, gains, s);
  return e == hipSuccess ? hipGetLastError() : e;
}

} // namespace

extern "C" {

int sip_lqr_plan_create(int dtype, int64_t batch, int T, int n, int m,
                        int device, sip_lqr_plan **plan) {
  return sip_lqr_plan_create_layout(dtype, batch, T, n, m, device, SIP_LQR_LAYOUT_FULL, plan);
}

int sip_lqr_plan_layout(const sip_lqr_plan *plan) { return plan ? plan->layout : SIP_LQR_LAYOUT_FULL; }

int sip_lqr_plan_create_layout(int dtype, int64_t batch, int T, int n, int m, int device, int layout,
                               sip_lqr_plan **plan) {
  if (plan == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  *plan = nullptr;
  if (batch < 1 || T < 0 || n < 1 || m < 1 ||
      (dtype != SIP_LQR_F64 && dtype != SIP_LQR_F32) ||
      (layout != SIP_LQR_LAYOUT_FULL && layout != SIP_LQR_LAYOUT_SYMMETRIC))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  const DispatchEnv env = dispatch_env();
  const KernelEntry *k = env.general ? nullptr : find_kernel(env, dtype, n, m, layout);
  if (layout != SIP_LQR_LAYOUT_FULL && k == nullptr)
    return SIP_LQR_ERR_UNSUPPORTED; // only the dedicated kernels read the packed triangles
  if (k == nullptr && env.variant != nullptr && !env.general)
    return SIP_LQR_ERR_UNSUPPORTED; // an explicitly requested variant does not exist
  bool embedded = false;
  if (k == nullptr && !env.general && dtype == SIP_LQR_F64 && env.pad) {
    k = find_embedding_kernel(env, n, m);
    embedded = k != nullptr;
  }
  sip_lqr_plan *p = new (std::nothrow) sip_lqr_plan;
  if (p == nullptr)
    return SIP_LQR_ERR_ALLOC;
  p->dtype = dtype;
  p->layout = layout;
  p->batch = batch;
  p->T = T;
  p->n = n;
  p->m = m;
  p->device = device;
  p->forced_general = env.general;
  init_generic(p);
  decide_kernel(p, k, embedded, env);
  // Device tables of the general engine: uploaded here, never lazily (include/sip_lqr_amd.h
  // promises that the compute entry points neither allocate nor synchronise).  A host without any
  // HIP device still gets a plan for the host-side entry points.
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess)
    ndev = 0;
  if (ndev > 0) {
    if (device < 0 || device >= ndev) {
      delete p;
      return SIP_LQR_ERR_INVALID_ARGUMENT;
    }
    const hipError_t e = p->gen.upload(device); // restores the caller's current device
    if (e != hipSuccess) {
      std::fprintf(stderr, "sip_lqr_plan_create: HIP error: %s\n", hipGetErrorString(e));
      delete p;
      return SIP_LQR_ERR_HIP;
    }
    p->on_device = true;
  } else {
    (void)hipGetLastError(); // hipErrorNoDevice is not sticky for the caller
  }
  *plan = p;
  return SIP_LQR_OK;
}

void sip_lqr_plan_destroy(sip_lqr_plan *plan) { delete plan; }

int sip_lqr_plan_set_separate_sweeps(sip_lqr_plan *plan, int on) {
  if (plan == nullptr || (on && plan->separate))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (!on || !plan->split_on_fused || plan->kernel->launch_factor_sweep == nullptr ||
      plan->kernel->launch_solve_sweep == nullptr)
    return SIP_LQR_OK; // the plan's kernel has no such sweeps (or its split calls run on the general engine)
  plan->separate = true;
  // the workspace stays what it was: the spill, the scratch of the split calls and the gfac region (M * M + M scalars
  // per edge) are those workspace_layout already reserves
  std::string name = std::string(plan->kernel_name) + plan->kernel->separate_suffix;
  plan->name_storage.swap(name);
  plan->kernel_name = plan->name_storage.c_str();
  return SIP_LQR_OK;
}

int sip_lqr_has_separate_sweeps(const sip_lqr_plan *plan) { return plan != nullptr && plan->separate ? 1 : 0; }

int sip_lqr_plan_set_fused_f32(sip_lqr_plan *plan, int on) {
  if (plan == nullptr || (on && plan->fused_f32))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (!on || plan->dtype != SIP_LQR_F32 || plan->layout != SIP_LQR_LAYOUT_FULL || plan->kernel != nullptr ||
      plan->forced_general)
    return SIP_LQR_OK; // not an fp32 plan of the general engine, or one that was asked to stay there
  const KernelEntry *row = nullptr;
  for (const KernelEntry &k : kQf32Rows)
    if (row == nullptr && k.n == plan->n && k.m == plan->m)
      row = &k;
  if (row == nullptr)
    return SIP_LQR_OK; // no fused fp32 kernel of this shape
  plan->fused_f32 = true;
  // factor and solve re-run the sweep (until sip_lqr_plan_set_separate_sweeps gives them sweeps of their own), unless
  // the split calls were asked to stay general; sip_lqr_workspace_bytes is the larger of the two layouts from here on,
  // as for every fused plan
  decide_kernel(plan, row, false, dispatch_env());
  return SIP_LQR_OK;
}

int sip_lqr_has_fused_f32(const sip_lqr_plan *plan) { return plan != nullptr && plan->fused_f32 ? 1 : 0; }

int sip_lqr_plan_set_wide_controls(sip_lqr_plan *plan, int on) {
  if (plan == nullptr || (on && plan->wide_controls))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (!on || plan->layout != SIP_LQR_LAYOUT_FULL || plan->kernel != nullptr || plan->forced_general || plan->m < 9 ||
      plan->m > 16 || plan->n > 32)
    return SIP_LQR_OK; // not a plan of the general engine with 9 to 16 controls, or one that was asked to stay there
  const KernelEntry *row = nullptr; // the row of the plan's dtype with the least M >= m
  for (const KernelEntry &k : kWideRows)
    if (row == nullptr && k.dtype == plan->dtype && k.m >= plan->m)
      row = &k;
  const DispatchEnv env = dispatch_env();
  const bool exact = plan->n == row->n && plan->m == row->m;
  if (!exact && (plan->dtype != SIP_LQR_F64 || !env.pad))
    return SIP_LQR_OK; // the embedding is fp64 only, and SIP_LQR_PAD=0 keeps the general engine, as at creation
  plan->wide_controls = true;
  decide_kernel(plan, row, !exact, env);
  return SIP_LQR_OK;
}

int sip_lqr_has_wide_controls(const sip_lqr_plan *plan) { return plan != nullptr && plan->wide_controls ? 1 : 0; }

int64_t sip_lqr_plan_batch(const sip_lqr_plan *p) { return p ? p->batch : 0; }
size_t sip_lqr_scalar_bytes(const sip_lqr_plan *p) { return p ? scalar_size(p) : 0; }
size_t sip_lqr_mats_len(const sip_lqr_plan *p) { return (size_t)lens(p).mats; }
size_t sip_lqr_vecs_len(const sip_lqr_plan *p) { return (size_t)lens(p).vecs; }
size_t sip_lqr_gains_len(const sip_lqr_plan *p) { return (size_t)lens(p).gains; }
size_t sip_lqr_mats_bytes(const sip_lqr_plan *p) {
  return (size_t)p->batch * sip_lqr_mats_len(p) * scalar_size(p);
}
size_t sip_lqr_vecs_bytes(const sip_lqr_plan *p) {
  return (size_t)p->batch * sip_lqr_vecs_len(p) * scalar_size(p);
}
size_t sip_lqr_sol_bytes(const sip_lqr_plan *p) {
  return sip_lqr_vecs_bytes(p);
}
size_t sip_lqr_gains_bytes(const sip_lqr_plan *p) {
  return (size_t)p->batch * sip_lqr_gains_len(p) * scalar_size(p);
}
size_t sip_lqr_status_bytes(const sip_lqr_plan *p) {
  return (size_t)p->batch * sizeof(int32_t);
}
size_t sip_lqr_workspace_bytes(const sip_lqr_plan *p) { return p->ws.total; }

} // extern "C"

namespace {
template <class S>
void pack_one(const sip_lqr_plan *pl, int64_t p, double *const *Q,
              double *const *M, double *const *R, double *const *q,
              double *const *r, double *const *A, double *const *B,
              double *const *c, double *const *delta, S *mats, S *vecs) {
  const int n = pl->n, m = pl->m, T = pl->T;
  S *mp = mats + (size_t)p * sip_lqr_mats_len(pl);
  S *vp = vecs + (size_t)p * sip_lqr_vecs_len(pl);
  auto put = [](S *&dst, const double *src, int count) {
    for (int i = 0; i < count; ++i)
      dst[i] = (S)src[i];
    dst += count;
  };
  const bool sym = pl->layout == SIP_LQR_LAYOUT_SYMMETRIC;
  auto put_lower = [](S *&dst, const double *src, int dim) { // lower triangle, packed by columns
    for (int col = 0; col < dim; ++col)
      for (int row = col; row < dim; ++row)
        *dst++ = (S)src[row + dim * col];
  };
  for (int i = 0; i <= T; ++i) {
    if (sym)
      put_lower(mp, Q[i], n);
    else
      put(mp, Q[i], n * n);
    put(mp, delta[i], n);
    put(vp, q[i], n);
    put(vp, c[i], n);
    if (i < T) {
      put(mp, A[i], n * n);
      put(mp, B[i], n * m);
      put(mp, M[i], n * m);
      if (sym)
        put_lower(mp, R[i], m);
      else
        put(mp, R[i], m * m);
      put(vp, r[i], m);
    }
  }
}

template <class S>
void unpack_sol(const sip_lqr_plan *pl, int64_t p, const S *sol,
                double *const *x, double *const *u, double *const *y) {
  const int n = pl->n, m = pl->m, T = pl->T;
  const S *sp = sol + (size_t)p * sip_lqr_vecs_len(pl);
  auto get = [](const S *&src, double *dst, int count) {
    for (int i = 0; i < count; ++i)
      dst[i] = (double)src[i];
    src += count;
  };
  for (int i = 0; i <= T; ++i) {
    get(sp, x[i], n);
    get(sp, y[i], n);
    if (i < T)
      get(sp, u[i], m);
  }
}

template <class S>
void unpack_gain(const sip_lqr_plan *pl, int64_t p, const S *gains,
                 double *const *K, double *const *k) {
  const int n = pl->n, m = pl->m, T = pl->T;
  const S *gp = gains + (size_t)p * sip_lqr_gains_len(pl);
  for (int i = 0; i < T; ++i) {
    for (int e = 0; e < m * n; ++e)
      K[i][e] = (double)gp[e];
    gp += m * n;
    for (int e = 0; e < m; ++e)
      k[i][e] = (double)gp[e];
    gp += m;
  }
}
} // namespace

extern "C" {

int sip_lqr_pack_problem(const sip_lqr_plan *plan, int64_t p, double *const *Q,
                         double *const *M, double *const *R, double *const *q,
                         double *const *r, double *const *A, double *const *B,
                         double *const *c, double *const *delta,
                         void *mats_host, void *vecs_host) {
  if (plan == nullptr || p < 0 || p >= plan->batch || !Q || !q || !c ||
      !delta || !mats_host || !vecs_host ||
      (plan->T > 0 && (!M || !R || !r || !A || !B)))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (plan->dtype == SIP_LQR_F32)
    pack_one<float>(plan, p, Q, M, R, q, r, A, B, c, delta, (float *)mats_host,
                    (float *)vecs_host);
  else
    pack_one<double>(plan, p, Q, M, R, q, r, A, B, c, delta,
                     (double *)mats_host, (double *)vecs_host);
  return SIP_LQR_OK;
}

int sip_lqr_unpack_solution(const sip_lqr_plan *plan, int64_t p,
                            const void *sol_host, double *const *x,
                            double *const *u, double *const *y) {
  if (plan == nullptr || p < 0 || p >= plan->batch || !sol_host || !x || !y ||
      (plan->T > 0 && !u))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (plan->dtype == SIP_LQR_F32)
    unpack_sol<float>(plan, p, (const float *)sol_host, x, u, y);
  else
    unpack_sol<double>(plan, p, (const double *)sol_host, x, u, y);
  return SIP_LQR_OK;
}

int sip_lqr_unpack_gains(const sip_lqr_plan *plan, int64_t p,
                         const void *gains_host, double *const *K,
                         double *const *k) {
  if (plan == nullptr || p < 0 || p >= plan->batch || !gains_host ||
      (plan->T > 0 && (!K || !k)))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (plan->dtype == SIP_LQR_F32)
    unpack_gain<float>(plan, p, (const float *)gains_host, K, k);
  else
    unpack_gain<double>(plan, p, (const double *)gains_host, K, k);
  return SIP_LQR_OK;
}

int sip_lqr_factor_solve(const sip_lqr_plan *plan, const void *d_mats,
                         const void *d_vecs, void *d_sol, void *d_gains,
                         int32_t *d_status, void *d_workspace, void *stream) {
  if (plan == nullptr || !d_mats || !d_vecs || !d_sol || !d_status ||
      !d_workspace || (plan->T > 0 && !d_gains))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  OnPlanDevice on_device(plan, "sip_lqr_factor_solve");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  if (plan->kernel != nullptr)
    return report(run_fused(plan, d_mats, d_vecs, d_sol, d_gains, d_status, d_workspace, s, Sweep::Full),
                  "sip_lqr_factor_solve");
  // no dedicated kernel for this shape / dtype: general engine, two launches
  hipError_t e = general_factor(plan, d_mats, d_workspace, d_gains, d_status, s);
  if (e == hipSuccess)
    e = general_solve(plan, d_mats, d_vecs, d_workspace, d_gains, d_sol, d_status, s);
  return report(e, "sip_lqr_factor_solve(general)");
}

// The fused sweep with A | B read in place (chain_qw16.hpp, SPLIT): staged fp64 kernels have it, for the plan's
// own shape only (not through the embedding).
int sip_lqr_has_split(const sip_lqr_plan *plan) { return plan != nullptr && plan->launch_split() != nullptr ? 1 : 0; }

int64_t sip_lqr_split_mats_len(const sip_lqr_plan *plan) { return plan ? lens(plan).split_mats : 0; }

int sip_lqr_factor_solve_split(const sip_lqr_plan *plan, const void *d_mats, const void *d_ab,
                               int64_t ab_problem_stride, int64_t ab_stage_stride, const void *d_vecs, void *d_sol,
                               void *d_gains, int32_t *d_status, void *d_workspace, void *stream) {
  if (plan == nullptr || !d_mats || !d_vecs || !d_sol || !d_status || !d_workspace ||
      (plan->T > 0 && (!d_gains || !d_ab)) || ab_problem_stride < 0 || ab_stage_stride < 0)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (!sip_lqr_has_split(plan))
    return SIP_LQR_ERR_UNSUPPORTED;
  // The staging code addresses the four problems of a wavefront by 32-bit byte offsets from the first
  // one's A | B: three problem strides plus one stage image must stay below 2^32 bytes.
  const uint64_t ab_block_bytes = ((uint64_t)plan->n * plan->n + (uint64_t)plan->n * plan->m) * 8u;
  if ((uint64_t)ab_problem_stride > (((uint64_t)1 << 32) - 1 - ab_block_bytes) / (3u * 8u))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice on_device(plan, "sip_lqr_factor_solve_split");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  return report(plan->launch_split()(plan->batch, plan->T, d_mats, d_ab, (long)ab_problem_stride,
                                     (long)ab_stage_stride, d_vecs, d_sol, d_gains, d_status, d_workspace,
                                     (hipStream_t)stream),
                "sip_lqr_factor_solve_split");
}

// Split entry points.  A plan with split_on_fused re-runs its fused sweep (or runs its separate sweeps); the others
// run the general engine, whose work arena holds the reference's factor state W, G_factor, V, F_factor,
// sqrt_delta(_inv), v.  Either way sip_lqr_factor keeps the statuses in the workspace for sip_lqr_solve.
int sip_lqr_factor(const sip_lqr_plan *plan, const void *d_mats, void *d_gains,
                   int32_t *d_status, void *d_workspace, void *stream) {
  if (plan == nullptr || !d_mats || !d_status || !d_workspace || (plan->T > 0 && !d_gains))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  OnPlanDevice on_device(plan, "sip_lqr_factor");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  const bool fused = plan->split_on_fused; // fused sweep on a zero right-hand side: K, statuses
  hipError_t e = fused ? run_fused(plan, d_mats, nullptr, nullptr, d_gains, d_status, d_workspace, s, Sweep::Factor)
                       : general_factor(plan, d_mats, d_workspace, d_gains, d_status, s);
  if (e == hipSuccess)
    e = sipamd::copy_async((char *)d_workspace + (fused ? plan->ws.status : plan->ws.general_status), d_status,
                           (size_t)plan->batch * sizeof(int32_t), s);
  return report(e, fused ? "sip_lqr_factor(fused)" : "sip_lqr_factor");
}

int sip_lqr_solve(const sip_lqr_plan *plan, const void *d_mats, const void *d_vecs, void *d_sol,
                  void *d_gains, void *d_workspace, void *stream) {
  if (plan == nullptr || !d_mats || !d_vecs || !d_sol || !d_workspace || (plan->T > 0 && !d_gains))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  OnPlanDevice on_device(plan, "sip_lqr_solve");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  char *w = (char *)d_workspace;
  if (plan->split_on_fused) // the fused sweep again, now with the right-hand side
    return report(run_fused(plan, d_mats, d_vecs, d_sol, d_gains, (int32_t *)(w + plan->ws.status), d_workspace, s,
                            plan->has_solve_mode() ? Sweep::Solve : Sweep::Full),
                  "sip_lqr_solve(fused)");
  return report(general_solve(plan, d_mats, d_vecs, d_workspace, d_gains, d_sol,
                              (const int32_t *)(w + plan->ws.general_status), s),
                "sip_lqr_solve");
}

size_t sip_lqr_solve_multi_workspace_bytes(const sip_lqr_plan *plan, int num_rhs) {
  if (plan == nullptr || num_rhs < 1)
    return 0;
  return (size_t)plan->batch * scalar_size(plan) * (size_t)column_sweep(plan, num_rhs).scalars;
}

int sip_lqr_solve_multi(const sip_lqr_plan *plan, const void *d_mats, const void *d_vecs_cols, void *d_sol_cols,
                        int num_rhs, void *d_gains, void *d_workspace, void *d_col_workspace, void *stream) {
  if (plan == nullptr || num_rhs < 0 || !d_mats || !d_workspace || (plan->T > 0 && !d_gains) ||
      (num_rhs > 0 && (!d_vecs_cols || !d_sol_cols)))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  const size_t col_bytes = sip_lqr_vecs_bytes(plan);
  const ColumnSweep cs = column_sweep(plan, num_rhs);
  if (cs.launch == nullptr) { // no column sweep for this plan
    for (int col = 0; col < num_rhs; ++col) {
      const int rc = sip_lqr_solve(plan, d_mats, (const char *)d_vecs_cols + (size_t)col * col_bytes,
                                   (char *)d_sol_cols + (size_t)col * col_bytes, d_gains, d_workspace, stream);
      if (rc != SIP_LQR_OK)
        return rc;
    }
    return SIP_LQR_OK;
  }
  if (num_rhs > 0 && d_col_workspace == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice on_device(plan, "sip_lqr_solve_multi");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  char *w = (char *)d_workspace;
  const long stride = (long)(col_bytes / scalar_size(plan));
  hipError_t e = hipSuccess;
  for (int col0 = 0; col0 < num_rhs && e == hipSuccess; col0 += cs.columns) {
    const int nc = std::min(cs.columns, num_rhs - col0);
    e = cs.launch(plan->batch, plan->T, d_mats, (const char *)d_vecs_cols + (size_t)col0 * col_bytes,
                  (char *)d_sol_cols + (size_t)col0 * col_bytes, d_gains, d_workspace, w + plan->ws.gfac,
                  d_col_workspace, (const int32_t *)(w + plan->ws.status), nc, stride, (hipStream_t)stream);
  }
  return report(e, plan->separate ? "sip_lqr_solve_multi(separate sweeps)" : "sip_lqr_solve_multi");
}

} // extern "C"

// ---- the residual of the chain KKT system and the refinement around the plan's solve (chain_residual.hpp), for one
// ---- column (sip_lqr_residual, sip_lqr_refine) and for several (sip_lqr_residual_multi, sip_lqr_refine_multi) -------
namespace {
// The regions of the refinement's scratch, in bytes: rho / s and d as [num_rhs][batch][vecs_len] in the plan's dtype,
// then s[c][p].
struct RefineWorkspace {
  size_t rho = 0, d = 0, scale = 0, total = 0;
};
RefineWorkspace refine_multi_layout(const sip_lqr_plan *p, int num_rhs) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t cols = num_rhs < 1 ? 0 : (size_t)num_rhs;
  const size_t vec = up(cols * (size_t)p->batch * (size_t)lens(p).vecs * scalar_size(p));
  RefineWorkspace w;
  w.d = vec;
  w.scale = 2 * vec;
  w.total = w.scale + up(cols * (size_t)p->batch * sizeof(double));
  return w;
}
RefineWorkspace refine_layout(const sip_lqr_plan *p) { return refine_multi_layout(p, 1); }

sipamd::residual::Args residual_args(const sip_lqr_plan *p, const void *mats, const void *vecs, const void *sol,
                                     bool wide) {
  sipamd::residual::Args a{};
  a.batch = (long)p->batch, a.T = p->T, a.n = p->n, a.m = p->m;
  a.f32 = p->dtype == SIP_LQR_F32;
  a.wide = wide;
  a.symmetric = p->layout == SIP_LQR_LAYOUT_SYMMETRIC;
  a.mats = mats, a.vecs = vecs, a.sol = sol;
  return a;
}

// The rounds of sip_lqr_refine and sip_lqr_refine_multi: scaled residual, solve(rho / s, d) -- the caller's solve of
// num_rhs columns, returning a SIP_LQR_* code --, sol64 += s d; then one plain residual for the norms of the result.
template <typename Solve>
int refine_rounds(const sip_lqr_plan *plan, const void *d_mats, const double *d_vecs64, double *d_sol64, int num_rhs,
                  int iterations, int from_zero, void *d_refine_workspace, const int32_t *d_status, double *d_norms,
                  hipStream_t s, const char *what, Solve solve) {
  const RefineWorkspace f = refine_multi_layout(plan, num_rhs);
  char *w = (char *)d_refine_workspace;
  double *scale = (double *)(w + f.scale);
  const long B = (long)plan->batch, len = lens(plan).vecs;
  const size_t row = (size_t)num_rhs * B; // norms of one round
  sipamd::residual::Args a = residual_args(plan, d_mats, d_vecs64, d_sol64, true);
  hipError_t e = from_zero ? sipamd::zero_async(d_sol64, row * len * sizeof(double), s) : hipSuccess;
  for (int j = 0; j < iterations && e == hipSuccess; ++j) {
    a.scaled = w + f.rho, a.scale = scale, a.norm = d_norms + (size_t)j * row;
    e = sipamd::residual::launch_residual_cols(a, num_rhs, s);
    if (e != hipSuccess)
      break;
    const int rc = solve(w + f.rho, w + f.d);
    if (rc != SIP_LQR_OK)
      return rc;
    e = sipamd::residual::launch_update_cols(num_rhs, B, len, plan->dtype == SIP_LQR_F32, w + f.d, scale, d_status,
                                             d_sol64, s);
  }
  if (e == hipSuccess) { // the norms of the result
    a.scaled = nullptr, a.scale = nullptr, a.norm = d_norms + (size_t)iterations * row;
    e = sipamd::residual::launch_residual_cols(a, num_rhs, s);
  }
  return report(e, what);
}
} // namespace

extern "C" {

int sip_lqr_residual(const sip_lqr_plan *plan, const void *d_mats, const void *d_vecs, const void *d_sol, int wide,
                     double *d_res, double *d_norm, void *stream) {
  if (plan == nullptr || !d_mats || !d_vecs || !d_sol || !d_norm || (wide != 0 && wide != 1))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice on_device(plan, "sip_lqr_residual");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  sipamd::residual::Args a = residual_args(plan, d_mats, d_vecs, d_sol, wide == 1);
  a.res = d_res;
  a.norm = d_norm;
  return report(sipamd::residual::launch_residual_cols(a, 1, (hipStream_t)stream), "sip_lqr_residual");
}

size_t sip_lqr_refine_workspace_bytes(const sip_lqr_plan *plan) { return plan ? refine_layout(plan).total : 0; }

int sip_lqr_refine(const sip_lqr_plan *plan, const void *d_mats, const double *d_vecs64, double *d_sol64,
                   int iterations, int from_zero, void *d_gains, void *d_workspace, void *d_refine_workspace,
                   const int32_t *d_status, double *d_norms, void *stream) {
  if (plan == nullptr || !d_mats || !d_vecs64 || !d_sol64 || !d_workspace || !d_refine_workspace || !d_norms ||
      (plan->T > 0 && !d_gains) || iterations < 1 || iterations > 32 || (from_zero != 0 && from_zero != 1))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice on_device(plan, "sip_lqr_refine");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  return refine_rounds(plan, d_mats, d_vecs64, d_sol64, 1, iterations, from_zero, d_refine_workspace, d_status, d_norms,
                       (hipStream_t)stream, "sip_lqr_refine", [&](const void *rho, void *d) {
                         return sip_lqr_solve(plan, d_mats, rho, d, d_gains, d_workspace, stream);
                       });
}

int sip_lqr_residual_multi_columns(const sip_lqr_plan *plan) {
  if (plan == nullptr)
    return 0;
  return sipamd::residual::cols_shape(plan->n, plan->m, plan->T, plan->dtype == SIP_LQR_F32,
                                      plan->layout == SIP_LQR_LAYOUT_SYMMETRIC, true, sipamd::residual::kColsMax)
      .columns;
}

int sip_lqr_residual_multi(const sip_lqr_plan *plan, const void *d_mats, const void *d_vecs_cols,
                           const void *d_sol_cols, int num_rhs, int wide, double *d_res_cols, double *d_norms,
                           void *stream) {
  if (plan == nullptr || !d_mats || !d_norms || num_rhs < 0 || (num_rhs > 0 && (!d_vecs_cols || !d_sol_cols)) ||
      (wide != 0 && wide != 1))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (num_rhs == 0)
    return SIP_LQR_OK;
  OnPlanDevice on_device(plan, "sip_lqr_residual_multi");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  sipamd::residual::Args a = residual_args(plan, d_mats, d_vecs_cols, d_sol_cols, wide == 1);
  a.res = d_res_cols;
  a.norm = d_norms;
  return report(sipamd::residual::launch_residual_cols(a, num_rhs, (hipStream_t)stream), "sip_lqr_residual_multi");
}

size_t sip_lqr_refine_multi_workspace_bytes(const sip_lqr_plan *plan, int num_rhs) {
  return plan ? refine_multi_layout(plan, num_rhs).total : 0;
}

int sip_lqr_refine_multi(const sip_lqr_plan *plan, const void *d_mats, const double *d_vecs64_cols,
                         double *d_sol64_cols, int num_rhs, int iterations, int from_zero, void *d_gains,
                         void *d_workspace, void *d_col_workspace, void *d_refine_workspace,
                         const int32_t *d_status, double *d_norms, void *stream) {
  if (plan == nullptr || !d_mats || !d_vecs64_cols || !d_sol64_cols || !d_workspace || !d_refine_workspace ||
      !d_norms || (plan->T > 0 && !d_gains) || iterations < 1 || iterations > 32 ||
      (from_zero != 0 && from_zero != 1) || num_rhs < 0 ||
      (!d_col_workspace && sip_lqr_solve_multi_workspace_bytes(plan, num_rhs) > 0))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (num_rhs == 0)
    return SIP_LQR_OK;
  OnPlanDevice on_device(plan, "sip_lqr_refine_multi");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  return refine_rounds(plan, d_mats, d_vecs64_cols, d_sol64_cols, num_rhs, iterations, from_zero, d_refine_workspace,
                       d_status, d_norms, (hipStream_t)stream, "sip_lqr_refine_multi", [&](const void *rho, void *d) {
                         return sip_lqr_solve_multi(plan, d_mats, rho, d, num_rhs, d_gains, d_workspace,
                                                    d_col_workspace, stream);
                       });
}

} // extern "C"

// ---- gradients of the solve: one adjoint solve and the outer-product kernel (chain_vjp.hpp) --------------------------
namespace {
sipamd::vjp::Args vjp_args(const sip_lqr_plan *p, const void *sol, const void *adj, bool wide, const int32_t *status,
                           void *grad) {
  sipamd::vjp::Args a{};
  a.batch = (long)p->batch, a.T = p->T, a.n = p->n, a.m = p->m;
  a.f32 = p->dtype == SIP_LQR_F32 && !wide;
  a.symmetric = p->layout == SIP_LQR_LAYOUT_SYMMETRIC;
  a.sol = sol, a.adj = adj, a.status = status, a.grad = grad;
  return a;
}
} // namespace

extern "C" {

int sip_lqr_vjp_mats(const sip_lqr_plan *plan, const void *d_sol, const void *d_adj, int wide,
                     const int32_t *d_status, void *d_grad_mats, void *stream) {
  if (plan == nullptr || !d_sol || !d_adj || !d_grad_mats || (wide != 0 && wide != 1))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice on_device(plan, "sip_lqr_vjp_mats");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  return report(sipamd::vjp::launch_vjp(vjp_args(plan, d_sol, d_adj, wide == 1, d_status, d_grad_mats),
                                        (hipStream_t)stream),
                "sip_lqr_vjp_mats");
}

int sip_lqr_vjp(const sip_lqr_plan *plan, const void *d_mats, const void *d_sol, const void *d_grad_sol,
                void *d_gains, void *d_workspace, const int32_t *d_status, void *d_grad_vecs, void *d_grad_mats,
                void *stream) {
  if (plan == nullptr || !d_mats || !d_sol || !d_grad_sol || !d_workspace || !d_grad_vecs ||
      (plan->T > 0 && !d_gains))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  // lambda: K lambda + g = 0 is the plan's solve with g as the right-hand side, and dL/dvecs as it stands
  const int rc = sip_lqr_solve(plan, d_mats, d_grad_sol, d_grad_vecs, d_gains, d_workspace, stream);
  if (rc != SIP_LQR_OK)
    return rc;
  if (d_status == nullptr && d_grad_mats == nullptr)
    return SIP_LQR_OK;
  OnPlanDevice on_device(plan, "sip_lqr_vjp");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  hipError_t e = hipSuccess;
  if (d_status != nullptr) // whatever the solve left for a failed problem
    e = sipamd::vjp::launch_mask((long)plan->batch, lens(plan).vecs, plan->dtype == SIP_LQR_F32, d_status,
                                 d_grad_vecs, (hipStream_t)stream);
  if (e == hipSuccess && d_grad_mats != nullptr)
    e = sipamd::vjp::launch_vjp(vjp_args(plan, d_sol, d_grad_vecs, false, d_status, d_grad_mats),
                                (hipStream_t)stream);
  return report(e, "sip_lqr_vjp");
}

} // extern "C"

// ---- the same for several columns: one adjoint solve_multi, and the columns summed in the kernel (chain_vjp_cols.hpp)
extern "C" {

int sip_lqr_vjp_multi_columns(const sip_lqr_plan *plan) {
  return plan ? sipamd::vjp::cols_per_launch(plan->n, plan->m) : 0;
}

int sip_lqr_vjp_mats_multi(const sip_lqr_plan *plan, const void *d_sol_cols, const void *d_adj_cols, int num_rhs,
                           int wide, const int32_t *d_status, void *d_grad_mats, void *stream) {
  if (plan == nullptr || num_rhs < 0 || (num_rhs > 0 && (!d_sol_cols || !d_adj_cols)) || !d_grad_mats ||
      (wide != 0 && wide != 1))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice on_device(plan, "sip_lqr_vjp_mats_multi");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  return report(sipamd::vjp::launch_vjp_cols(vjp_args(plan, d_sol_cols, d_adj_cols, wide == 1, d_status, d_grad_mats),
                                             num_rhs, (hipStream_t)stream),
                "sip_lqr_vjp_mats_multi");
}

int sip_lqr_vjp_multi(const sip_lqr_plan *plan, const void *d_mats, const void *d_sol_cols,
                      const void *d_grad_sol_cols, int num_rhs, void *d_gains, void *d_workspace,
                      void *d_col_workspace, const int32_t *d_status, void *d_grad_vecs_cols, void *d_grad_mats,
                      void *stream) {
  if (plan == nullptr || num_rhs < 0 || !d_mats || !d_workspace || !d_grad_vecs_cols || (plan->T > 0 && !d_gains) ||
      (num_rhs > 0 && (!d_sol_cols || !d_grad_sol_cols)) ||
      (!d_col_workspace && sip_lqr_solve_multi_workspace_bytes(plan, num_rhs) > 0))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  // lambda_c: K lambda_c + g_c = 0 is the plan's solve_multi with the g columns as the right-hand sides
  const int rc = sip_lqr_solve_multi(plan, d_mats, d_grad_sol_cols, d_grad_vecs_cols, num_rhs, d_gains, d_workspace,
                                     d_col_workspace, stream);
  if (rc != SIP_LQR_OK)
    return rc;
  if ((d_status == nullptr || num_rhs == 0) && d_grad_mats == nullptr)
    return SIP_LQR_OK;
  OnPlanDevice on_device(plan, "sip_lqr_vjp_multi");
  if (on_device.rc != SIP_LQR_OK)
    return on_device.rc;
  hipError_t e = hipSuccess;
  if (d_status != nullptr && num_rhs > 0) // whatever the solves left for a failed problem, in every column
    e = sipamd::vjp::launch_mask_cols(num_rhs, (long)plan->batch, lens(plan).vecs, plan->dtype == SIP_LQR_F32,
                                      d_status, d_grad_vecs_cols, (hipStream_t)stream);
  if (e == hipSuccess && d_grad_mats != nullptr)
    e = sipamd::vjp::launch_vjp_cols(vjp_args(plan, d_sol_cols, d_grad_vecs_cols, false, d_status, d_grad_mats),
                                     num_rhs, (hipStream_t)stream);
  return report(e, "sip_lqr_vjp_multi");
}

} // extern "C"

extern "C" {

const char *sip_lqr_kernel_name(const sip_lqr_plan *plan) {
  return plan ? plan->kernel_name : "";
}

// "sip_lqr_amd <version> (gfx950) SIPLQRSRC=<sha256 of the sources and flags the library was built
// from>": __graft_entry__.build_hip() links the stamp in and rebuilds when it differs from the sources
// next to the library; bench.py and smoke() print it, so that a run record names the build it measured.
const char *sip_lqr_version(void) {
  static const std::string v = std::string("sip_lqr_amd 0.2 (gfx950) ") + sip_lqr_build_stamp;
  return v.c_str();
}

} // extern "C"
