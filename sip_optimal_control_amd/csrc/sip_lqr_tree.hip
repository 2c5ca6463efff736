// sip_lqr_tree.hip -- C ABI of the general tree / variable-dimension path
// (include/sip_lqr_amd.h, second half): the general engine (generic_plan.hpp
// over tree_generic.hpp) and, where a size class holds the tree, the fused
// kernels (tree_qw16_launch.hpp).  What a plan decides on the host:
// tree_plan.hpp; here its device tables, the argument checks and the launches.
#include "../../include/sip_lqr_amd.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <new>
#include <vector>

#include "generic_plan.hpp"
#include "residual_launch.hpp"
#include "table_packer.hpp"
#include "tree_plan.hpp"
#include "tree_residual_cols_launch.hpp"
#include "tree_vjp_cols_launch.hpp"
#include "tree_vjp_launch.hpp"
#include "vjp_cols_launch.hpp"
#include "vjp_launch.hpp"

struct sip_lqr_tree_plan {
  int64_t batch = 0;
  int device = 0;
  int topology_status = SIP_LQR_INVALID_TOPOLOGY;
  sipamd::GenericPlan g;
  // fused factor + solve on the padded size class (tree_qw16.hpp); nullptr: general engine only
  const sipamd::TreeClass *fused = nullptr;
  sipamd::TreeSchedule sched{};
  void *d_steps = nullptr;
  sipamd::TreeScratch scratch; // of the fused kernels: padded gains at 0, then the spill
  sipamd::residual::TreeColsDims residual_cols; // what the launch shape of the residual kernel reads of the plan
  void *d_vjp_table = nullptr; // of the gradient kernel (tree_vjp_table.hpp): one word per input-arena scalar
  ~sip_lqr_tree_plan() {
    if (d_steps != nullptr)
      (void)hipFree(d_steps);
    if (d_vjp_table != nullptr)
      (void)hipFree(d_vjp_table);
  }
};

namespace {

using sipamd::report;

// The flattened traversal on the plan's device, p->sched pointing at it.
hipError_t upload_schedule(sip_lqr_tree_plan *p) {
  sipamd::HostTreeSchedule h = sipamd::build_tree_schedule(p->g);
  p->sched = h.sched;
  sipamd::TablePacker<sipamd::TreeStep> steps;
  steps.push(h.backward, &p->sched.backward), steps.push(h.forward, &p->sched.forward);
  sipamd::DeviceGuard on_device(p->device);
  return on_device.err != hipSuccess ? on_device.err : steps.upload(&p->d_steps);
}

// The table of the gradient kernel on the plan's device.
hipError_t upload_vjp_table(sip_lqr_tree_plan *p) {
  sipamd::TablePacker<sipamd::tree_vjp::Word> words;
  words.push(sipamd::tree_vjp::build_table(p->g));
  sipamd::DeviceGuard on_device(p->device);
  return on_device.err != hipSuccess ? on_device.err : words.upload(&p->d_vjp_table);
}

// The preamble of a compute entry point: the plan's device is the current one while this lives, whatever the
// caller's (which is restored).  rc != SIP_LQR_OK: to be returned.
struct OnPlanDevice {
  sipamd::DeviceGuard guard;
  hipStream_t s;
  int rc;
  OnPlanDevice(const sip_lqr_tree_plan *p, void *stream)
      : guard(p->device), s((hipStream_t)stream), rc(guard.err == hipSuccess ? SIP_LQR_OK : SIP_LQR_ERR_HIP) {}
};

// Served by the general engine's entry points: a latched topology status, or no size class.
bool general_engine(const sip_lqr_tree_plan *p) { return p->topology_status != SIP_LQR_SUCCESS || p->fused == nullptr; }
bool missing_input(const sip_lqr_tree_plan *p, const double *d_input) { return d_input == nullptr && p->g.in0_len > 0; }
bool missing_output(const sip_lqr_tree_plan *p, const double *d_output) { return d_output == nullptr && p->g.out_len > 0; }
double *spill_of(const sip_lqr_tree_plan *p, void *d_scratch) { return (double *)((char *)d_scratch + p->scratch.at_spill); }

} // namespace

extern "C" {

int sip_lqr_compile_topology(int num_edges, int root, const int *edge_parents,
                             const int *edge_children, int *child_offsets,
                             int *child_edges, int *edge_parents_out,
                             int *edge_children_out, int *preorder,
                             int *postorder, int *node_marks) {
  return sipamd::compile_topology(num_edges, root, edge_parents, edge_children, child_offsets, child_edges,
                                  edge_parents_out, edge_children_out, preorder, postorder, node_marks);
}

int sip_lqr_tree_plan_create(int64_t batch, int num_edges, int root,
                             const int *edge_parents, const int *edge_children,
                             const int *state_dims, const int *control_dims,
                             int device, sip_lqr_tree_plan **out) {
  // validate
  if (out == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (batch < 1 || num_edges < 0 || state_dims == nullptr ||
      (num_edges > 0 && control_dims == nullptr))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  const int E = num_edges, N = E + 1;
  for (int i = 0; i < N; ++i)
    if (state_dims[i] < 0)
      return SIP_LQR_ERR_INVALID_ARGUMENT;
  for (int e = 0; e < E; ++e)
    if (control_dims[e] < 0)
      return SIP_LQR_ERR_INVALID_ARGUMENT;
  sip_lqr_tree_plan *p = new (std::nothrow) sip_lqr_tree_plan;
  if (p == nullptr)
    return SIP_LQR_ERR_ALLOC;
  p->batch = batch;
  p->device = device;
  *out = p;
  // topology
  sipamd::GenericPlan &g = p->g;
  g.set_shape(E, root, state_dims, control_dims);
  p->topology_status = g.compile(edge_parents, edge_children);
  if (p->topology_status != SIP_LQR_SUCCESS)
    return SIP_LQR_OK; // latched, reported by factor (lqr.cpp:646-648)
  // layout, upload
  g.layout_tree_native();
  hipError_t e = g.upload(device);
  if (e == hipSuccess)
    e = upload_vjp_table(p);
  p->residual_cols = sipamd::residual::tree_cols_dims(N, E, g.state_dims.data(), g.control_dims.data(),
                                                      g.parents.data(), g.children.data());
  // size class of the fused kernels; where one holds the tree: its schedule and its scratch
  if (e == hipSuccess)
    p->fused = sipamd::choose_tree_class(g);
  if (p->fused != nullptr) {
    e = upload_schedule(p);
    p->scratch = sipamd::partition_tree_scratch(*p->fused, batch, N, E);
  }
  if (e != hipSuccess) {
    std::fprintf(stderr, "sip_lqr_tree_plan_create: HIP error: %s\n", hipGetErrorString(e));
    delete p;
    *out = nullptr;
    return SIP_LQR_ERR_HIP;
  }
  return SIP_LQR_OK;
}

void sip_lqr_tree_plan_destroy(sip_lqr_tree_plan *plan) { delete plan; }

int sip_lqr_tree_topology_status(const sip_lqr_tree_plan *plan) {
  return plan ? plan->topology_status : SIP_LQR_INVALID_TOPOLOGY;
}

const int *sip_lqr_tree_topology_array(const sip_lqr_tree_plan *plan, int which) {
  if (plan == nullptr)
    return nullptr;
  switch (which) {
  case 0: return plan->g.child_offsets.data();
  case 1: return plan->g.child_edges.data();
  case 2: return plan->g.preorder.data();
  case 3: return plan->g.postorder.data();
  default: return nullptr;
  }
}

size_t sip_lqr_tree_input_len(const sip_lqr_tree_plan *p) { return p ? (size_t)p->g.in0_len : 0; }
size_t sip_lqr_tree_work_len(const sip_lqr_tree_plan *p) { return p ? (size_t)p->g.ws_len : 0; }
size_t sip_lqr_tree_output_len(const sip_lqr_tree_plan *p) { return p ? (size_t)p->g.out_len : 0; }

size_t sip_lqr_tree_offset(const sip_lqr_tree_plan *p, int arena, int kind, int index) {
  if (p == nullptr || p->topology_status != SIP_LQR_SUCCESS || arena < 0 || arena > 2 ||
      kind < 0 || kind > 1 || index < 0 || index >= (kind == 0 ? p->g.N : p->g.E))
    return (size_t)-1;
  // first block of each (arena, kind) group: Q.. / A.. ; W.. / V.. ; x.. / u
  const std::vector<long> *tab[3][2] = {{&p->g.oQ, &p->g.oA}, {&p->g.oV, &p->g.oW}, {&p->g.ox, &p->g.ou}};
  return (size_t)(*tab[arena][kind])[index];
}

int sip_lqr_tree_factor(const sip_lqr_tree_plan *plan, const double *d_input,
                        double *d_work, int32_t *d_status, void *stream) {
  if (plan == nullptr || d_status == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  if (plan->topology_status != SIP_LQR_SUCCESS) {
    // every instance reports the latched traversal status (lqr.cpp:646-648)
    // (a copy from host memory and a wait: the one place of the library that does not only enqueue kernels)
    std::vector<int32_t> st((size_t)plan->batch, plan->topology_status);
    if (hipMemcpyAsync(d_status, st.data(), st.size() * sizeof(int32_t), hipMemcpyHostToDevice, dev.s) != hipSuccess ||
        hipStreamSynchronize(dev.s) != hipSuccess)
      return SIP_LQR_ERR_HIP;
    return SIP_LQR_OK;
  }
  if (missing_input(plan, d_input) || d_work == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  return report(plan->g.launch_factor<double>((long)plan->batch, d_input, d_work, d_work, d_status, dev.s),
                "sip_lqr_tree_factor");
}

int sip_lqr_tree_solve(const sip_lqr_tree_plan *plan, const double *d_input,
                       double *d_work, double *d_output, const int32_t *d_status,
                       void *stream) {
  if (plan == nullptr || d_status == nullptr || d_work == nullptr || missing_output(plan, d_output) ||
      missing_input(plan, d_input))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (plan->topology_status != SIP_LQR_SUCCESS)
    return SIP_LQR_ERR_INVALID_ARGUMENT; // solve() needs a successful factor
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  return report(plan->g.launch_solve<double>((long)plan->batch, d_input, d_input, d_work, d_work, d_output, d_status,
                                             dev.s),
                "sip_lqr_tree_solve");
}

size_t sip_lqr_tree_rhs_len(const sip_lqr_tree_plan *p) { return p ? (size_t)p->g.out_len : 0; }

size_t sip_lqr_tree_rhs_offset(const sip_lqr_tree_plan *p, int kind, int index) {
  // the output arena's layout: q | c where x | y are, r where u is
  return sip_lqr_tree_offset(p, 2, kind, index);
}

size_t sip_lqr_tree_solve_multi_scratch_bytes(const sip_lqr_tree_plan *p, int num_rhs) {
  if (p == nullptr || num_rhs < 1 || p->topology_status != SIP_LQR_SUCCESS)
    return 0;
  const size_t B = (size_t)p->batch * sizeof(double);
  if (p->fused != nullptr)
    return B * (size_t)num_rhs * (size_t)p->fused->cols_len(p->sched);
  return B * (size_t)p->g.cols_len(); // the general engine: one column's worth, reused by every column
}

int sip_lqr_tree_solve_multi(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work,
                             const double *d_rhs_cols, double *d_out_cols, int num_rhs, const int32_t *d_status,
                             void *d_scratch, void *stream) {
  if (plan == nullptr || num_rhs < 1 || d_status == nullptr || d_work == nullptr || d_scratch == nullptr ||
      ((d_rhs_cols == nullptr || d_out_cols == nullptr) && plan->g.out_len > 0) || missing_input(plan, d_input))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (plan->topology_status != SIP_LQR_SUCCESS)
    return SIP_LQR_ERR_INVALID_ARGUMENT; // solve() needs a successful factor
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  const long batch = (long)plan->batch;
  const hipError_t e =
      plan->fused != nullptr // all columns in one launch (tree_mrhs_qw16.hpp); else column by column
          ? plan->fused->launch_multi(plan->sched, d_input, d_work, d_rhs_cols, d_out_cols, (double *)d_scratch,
                                      d_status, batch, num_rhs, dev.s)
          : plan->g.launch_solve_cols<double>(batch, d_input, d_work, d_rhs_cols, d_out_cols, num_rhs,
                                              (double *)d_scratch, d_status, dev.s);
  return report(e, "sip_lqr_tree_solve_multi");
}

const char *sip_lqr_tree_multi_kernel_name(const sip_lqr_tree_plan *plan) {
  if (plan == nullptr)
    return "";
  return plan->fused != nullptr ? plan->fused->multi_name : "tree_generic/f64 column by column";
}

const char *sip_lqr_tree_kernel_name(const sip_lqr_tree_plan *plan) {
  if (plan == nullptr)
    return "";
  return plan->fused != nullptr ? plan->fused->name : "tree_generic/f64";
}

size_t sip_lqr_tree_fused_scratch_bytes(const sip_lqr_tree_plan *plan) {
  return (plan != nullptr && plan->fused != nullptr) ? plan->scratch.bytes : 0;
}

namespace {
int tree_factor_solve_impl(const sip_lqr_tree_plan *plan, const double *d_input, double *d_work, double *d_output,
                           int32_t *d_status, void *d_scratch, void *stream, const bool workspace) {
  if (plan == nullptr || d_status == nullptr || (workspace && d_work == nullptr))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (general_engine(plan)) { // two launches
    const int rc = sip_lqr_tree_factor(plan, d_input, d_work, d_status, stream);
    if (rc != SIP_LQR_OK || plan->topology_status != SIP_LQR_SUCCESS)
      return rc;
    return sip_lqr_tree_solve(plan, d_input, d_work, d_output, d_status, stream);
  }
  if (missing_input(plan, d_input) || missing_output(plan, d_output) || d_scratch == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  const auto launch = workspace ? plan->fused->launch_export : plan->fused->launch;
  return report(launch(plan->sched, d_input, d_output, d_work, (double *)d_scratch, spill_of(plan, d_scratch),
                       d_status, (long)plan->batch, dev.s),
                "sip_lqr_tree_factor_solve");
}
} // namespace

int sip_lqr_tree_factor_solve(const sip_lqr_tree_plan *plan, const double *d_input, double *d_work, double *d_output,
                              int32_t *d_status, void *d_scratch, void *stream) {
  return tree_factor_solve_impl(plan, d_input, d_work, d_output, d_status, d_scratch, stream, false);
}

int sip_lqr_tree_factor_solve_workspace(const sip_lqr_tree_plan *plan, const double *d_input, double *d_work,
                                        double *d_output, int32_t *d_status, void *d_scratch, void *stream) {
  return tree_factor_solve_impl(plan, d_input, d_work, d_output, d_status, d_scratch, stream, true);
}

int sip_lqr_tree_factor_fused(const sip_lqr_tree_plan *plan, const double *d_input, double *d_work,
                              int32_t *d_status, void *d_scratch, void *stream) {
  if (plan == nullptr || d_status == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (general_engine(plan)) // (a latched status: reported by it)
    return sip_lqr_tree_factor(plan, d_input, d_work, d_status, stream);
  if (missing_input(plan, d_input) || d_work == nullptr || d_scratch == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  return report(plan->fused->launch_factor(plan->sched, d_input, d_work, (double *)d_scratch,
                                           spill_of(plan, d_scratch), d_status, (long)plan->batch, dev.s),
                "sip_lqr_tree_factor_fused");
}

int sip_lqr_tree_solve_fused(const sip_lqr_tree_plan *plan, const double *d_input, double *d_work, double *d_output,
                             const int32_t *d_status, void *d_scratch, void *stream) {
  if (plan == nullptr || d_status == nullptr || d_work == nullptr || missing_output(plan, d_output) ||
      missing_input(plan, d_input))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (plan->topology_status != SIP_LQR_SUCCESS)
    return SIP_LQR_ERR_INVALID_ARGUMENT; // solve() needs a successful factor
  if (general_engine(plan))
    return sip_lqr_tree_solve(plan, d_input, d_work, d_output, d_status, stream);
  if (d_scratch == nullptr) // (unused by the solve, but part of the contract: the plan's fused scratch)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  return report(plan->fused->launch_solve(plan->sched, d_input, d_work, d_output, d_status, (long)plan->batch, dev.s),
                "sip_lqr_tree_solve_fused");
}

const char *sip_lqr_tree_split_kernel_name(const sip_lqr_tree_plan *plan) {
  if (plan == nullptr)
    return "";
  return plan->fused != nullptr ? plan->fused->split_name : "tree_generic/f64";
}

// ---- the residual of the tree KKT system and the refinement around the plan's solve (tree_residual.hpp), for one
// ---- column (sip_lqr_tree_residual, sip_lqr_tree_refine) and for several (..._multi) --------------------------------
} // extern "C"

namespace {
// The regions of the refinement's scratch, in bytes: rho / s and d as [num_rhs][batch][rhs_len], s[c][p], then the
// scratch of the solve of num_rhs columns.
struct TreeRefineWorkspace {
  size_t d = 0, scale = 0, solve = 0, total = 0; // rho / s is at 0
};
TreeRefineWorkspace tree_refine_multi_layout(const sip_lqr_tree_plan *p, int num_rhs) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t cols = (size_t)num_rhs;
  const size_t vec = up(cols * (size_t)p->batch * (size_t)p->g.out_len * sizeof(double));
  TreeRefineWorkspace w;
  w.d = vec;
  w.scale = 2 * vec;
  w.solve = w.scale + up(cols * (size_t)p->batch * sizeof(double));
  w.total = w.solve + up(sip_lqr_tree_solve_multi_scratch_bytes(p, num_rhs));
  return w;
}
TreeRefineWorkspace tree_refine_layout(const sip_lqr_tree_plan *p) { return tree_refine_multi_layout(p, 1); }

sipamd::residual::TreeColsShape residual_shape(const sip_lqr_tree_plan *p, int requested) {
  return sipamd::residual::tree_cols_shape(p->residual_cols, true, requested);
}
bool valid_plan(const sip_lqr_tree_plan *p) { return p != nullptr && p->topology_status == SIP_LQR_SUCCESS; }

// sip_lqr_tree_residual and sip_lqr_tree_residual_multi behind their checks
int tree_residual(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_rhs_cols,
                  const double *d_out_cols, int num_rhs, double *d_res_cols, double *d_norms, void *stream,
                  const char *what) {
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  sipamd::residual::TreeColsArgs a{};
  a.batch = (long)plan->batch, a.input = d_input, a.rhs_cols = d_rhs_cols, a.sol_cols = d_out_cols;
  a.res = d_res_cols, a.norm = d_norms;
  return report(sipamd::residual::launch_tree_residual_cols(plan->g.meta, plan->residual_cols, a, num_rhs, dev.s), what);
}

// sip_lqr_tree_refine and sip_lqr_tree_refine_multi behind their checks: `iterations` rounds of scaled residual,
// sip_lqr_tree_solve_multi on rho / s, out += s d; then one plain residual for the norms of the result.
int tree_refine(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work, const double *d_rhs_cols,
                double *d_out_cols, int num_rhs, int iterations, int from_zero, const int32_t *d_status,
                void *d_refine_workspace, double *d_norms, void *stream, const char *what) {
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  const TreeRefineWorkspace f = tree_refine_multi_layout(plan, num_rhs);
  char *w = (char *)d_refine_workspace;
  double *rho = (double *)w, *d = (double *)(w + f.d), *scale = (double *)(w + f.scale);
  const long B = (long)plan->batch, len = plan->g.out_len;
  const size_t row = (size_t)num_rhs * B; // norms of one round
  sipamd::residual::TreeColsArgs a{};
  a.batch = B, a.input = d_input, a.rhs_cols = d_rhs_cols, a.sol_cols = d_out_cols;
  auto residual = [&]() {
    return sipamd::residual::launch_tree_residual_cols(plan->g.meta, plan->residual_cols, a, num_rhs, dev.s);
  };
  hipError_t e = from_zero ? sipamd::zero_async(d_out_cols, row * len * sizeof(double), dev.s) : hipSuccess;
  for (int j = 0; j < iterations && e == hipSuccess; ++j) {
    a.scaled = rho, a.scale = scale, a.norm = d_norms + (size_t)j * row;
    e = residual();
    if (e != hipSuccess)
      break;
    // (an empty output arena: rho and d have no entries, and the solve's check of them does not apply)
    const int rc = sip_lqr_tree_solve_multi(plan, d_input, d_work, rho, d, num_rhs, d_status, w + f.solve, stream);
    if (rc != SIP_LQR_OK)
      return rc;
    e = sipamd::residual::launch_update_cols(num_rhs, B, len, false, d, scale, d_status, d_out_cols, dev.s);
  }
  if (e == hipSuccess) { // the norms of the result
    a.scaled = nullptr, a.scale = nullptr, a.norm = d_norms + (size_t)iterations * row;
    e = residual();
  }
  return report(e, what);
}
} // namespace

extern "C" {

const char *sip_lqr_tree_residual_kernel_name(const sip_lqr_tree_plan *plan) {
  if (plan == nullptr)
    return "";
  // (a latched topology: its dimensions were never read, and the name stays the one such a plan always reported)
  return valid_plan(plan) && residual_shape(plan, 1).staged ? "tree_residual<staged>/f64" : "tree_residual<direct>/f64";
}

int sip_lqr_tree_residual(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_rhs,
                          const double *d_output, double *d_res, double *d_norm, void *stream) {
  if (plan == nullptr || d_norm == nullptr || missing_input(plan, d_input) || missing_output(plan, d_output) ||
      plan->topology_status != SIP_LQR_SUCCESS)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  return tree_residual(plan, d_input, d_rhs, d_output, 1, d_res, d_norm, stream, "sip_lqr_tree_residual");
}

size_t sip_lqr_tree_refine_workspace_bytes(const sip_lqr_tree_plan *plan) {
  return valid_plan(plan) ? tree_refine_layout(plan).total : 0;
}

int sip_lqr_tree_refine(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work, const double *d_rhs,
                        double *d_output, int iterations, int from_zero, const int32_t *d_status,
                        void *d_refine_workspace, double *d_norms, void *stream) {
  if (plan == nullptr || d_status == nullptr || d_work == nullptr || d_refine_workspace == nullptr ||
      d_norms == nullptr || missing_input(plan, d_input) || missing_output(plan, d_output) || iterations < 1 ||
      iterations > 32 || (from_zero != 0 && from_zero != 1) || plan->topology_status != SIP_LQR_SUCCESS)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  return tree_refine(plan, d_input, d_work, d_rhs, d_output, 1, iterations, from_zero, d_status, d_refine_workspace,
                     d_norms, stream, "sip_lqr_tree_refine");
}

int sip_lqr_tree_residual_multi_columns(const sip_lqr_tree_plan *plan) {
  return valid_plan(plan) ? residual_shape(plan, sipamd::residual::kTreeColsMax).columns : 0;
}

const char *sip_lqr_tree_residual_multi_kernel_name(const sip_lqr_tree_plan *plan) {
  if (!valid_plan(plan)) // (a latched topology: no launch, no kernel)
    return "";
  static const char *const names[2][4] = {
      {"tree_residual_cols<direct,1>/f64", "tree_residual_cols<direct,2>/f64", "tree_residual_cols<direct,4>/f64",
       "tree_residual_cols<direct,8>/f64"},
      {"tree_residual_cols<staged,1>/f64", "tree_residual_cols<staged,2>/f64", "tree_residual_cols<staged,4>/f64",
       "tree_residual_cols<staged,8>/f64"}};
  const sipamd::residual::TreeColsShape sh = residual_shape(plan, sipamd::residual::kTreeColsMax);
  const int k = sh.columns >= 8 ? 3 : (sh.columns >= 4 ? 2 : (sh.columns >= 2 ? 1 : 0));
  return names[sh.staged ? 1 : 0][k];
}

int sip_lqr_tree_residual_multi(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_rhs_cols,
                                const double *d_out_cols, int num_rhs, double *d_res_cols, double *d_norms,
                                void *stream) {
  if (plan == nullptr || d_norms == nullptr || num_rhs < 0 || missing_input(plan, d_input) ||
      (num_rhs > 0 && missing_output(plan, d_out_cols)) || plan->topology_status != SIP_LQR_SUCCESS)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (num_rhs == 0)
    return SIP_LQR_OK;
  return tree_residual(plan, d_input, d_rhs_cols, d_out_cols, num_rhs, d_res_cols, d_norms, stream,
                       "sip_lqr_tree_residual_multi");
}

size_t sip_lqr_tree_refine_multi_workspace_bytes(const sip_lqr_tree_plan *plan, int num_rhs) {
  return valid_plan(plan) && num_rhs >= 1 ? tree_refine_multi_layout(plan, num_rhs).total : 0;
}

int sip_lqr_tree_refine_multi(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work,
                              const double *d_rhs_cols, double *d_out_cols, int num_rhs, int iterations, int from_zero,
                              const int32_t *d_status, void *d_refine_workspace, double *d_norms, void *stream) {
  if (plan == nullptr || d_status == nullptr || d_work == nullptr || d_refine_workspace == nullptr ||
      d_norms == nullptr || num_rhs < 0 || missing_input(plan, d_input) ||
      (num_rhs > 0 && missing_output(plan, d_out_cols)) || iterations < 1 || iterations > 32 ||
      (from_zero != 0 && from_zero != 1) || plan->topology_status != SIP_LQR_SUCCESS)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (num_rhs == 0)
    return SIP_LQR_OK;
  return tree_refine(plan, d_input, d_work, d_rhs_cols, d_out_cols, num_rhs, iterations, from_zero, d_status,
                     d_refine_workspace, d_norms, stream, "sip_lqr_tree_refine_multi");
}

} // extern "C"

// ---- gradients of the solve: one adjoint solve and the outer-product kernel (tree_vjp.hpp) --------------------------
namespace {
sipamd::tree_vjp::Args tree_vjp_args(const sip_lqr_tree_plan *p, const double *sol, const double *adj,
                                     const int32_t *status, double *grad) {
  sipamd::tree_vjp::Args a{};
  a.batch = (long)p->batch, a.in_len = p->g.in0_len, a.out_len = p->g.out_len;
  a.table = (const sipamd::tree_vjp::Word *)p->d_vjp_table;
  a.sol = sol, a.adj = adj, a.status = status, a.grad = grad;
  return a;
}
} // namespace

extern "C" {

const char *sip_lqr_tree_vjp_kernel_name(const sip_lqr_tree_plan *plan) {
  if (!valid_plan(plan)) // (a latched topology: no table, no kernel)
    return "";
  return sipamd::tree_vjp::kernel_name(
      sipamd::tree_vjp::launch_shape(plan->g.in0_len, plan->g.out_len, (long)plan->batch));
}

int sip_lqr_tree_vjp_input(const sip_lqr_tree_plan *plan, const double *d_output, const double *d_adj,
                           const int32_t *d_status, double *d_grad_input, void *stream) {
  if (!valid_plan(plan) || missing_output(plan, d_output) || missing_output(plan, d_adj) ||
      missing_input(plan, d_grad_input))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  return report(sipamd::tree_vjp::launch_tree_vjp(tree_vjp_args(plan, d_output, d_adj, d_status, d_grad_input), dev.s),
                "sip_lqr_tree_vjp_input");
}

size_t sip_lqr_tree_vjp_scratch_bytes(const sip_lqr_tree_plan *plan) {
  return sip_lqr_tree_solve_multi_scratch_bytes(plan, 1);
}

int sip_lqr_tree_vjp(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work,
                     const double *d_output, const double *d_grad_output, const int32_t *d_status, double *d_adj,
                     double *d_grad_input, void *d_scratch, void *stream) {
  if (!valid_plan(plan) || d_status == nullptr || d_work == nullptr || d_scratch == nullptr ||
      missing_input(plan, d_input) || missing_output(plan, d_grad_output) || missing_output(plan, d_adj) ||
      (d_grad_input != nullptr && missing_output(plan, d_output)))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  // lambda: K lambda + g = 0 is the plan's one-column solve with g as the right-hand side, and dL/d(q, c, r) as it stands
  const int rc = sip_lqr_tree_solve_multi(plan, d_input, d_work, d_grad_output, d_adj, 1, d_status, d_scratch, stream);
  if (rc != SIP_LQR_OK)
    return rc;
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  hipError_t e = hipSuccess;
  if (plan->g.out_len > 0) // the solve leaves a failed problem's column untouched
    e = sipamd::vjp::launch_mask((long)plan->batch, plan->g.out_len, false, d_status, d_adj, dev.s);
  if (e == hipSuccess && d_grad_input != nullptr)
    e = sipamd::tree_vjp::launch_tree_vjp(tree_vjp_args(plan, d_output, d_adj, d_status, d_grad_input), dev.s);
  return report(e, "sip_lqr_tree_vjp");
}

// ---- several columns against one input arena, one gradient (tree_vjp_cols.hpp) -------------------------------------

int sip_lqr_tree_vjp_multi_columns(const sip_lqr_tree_plan *plan) {
  return valid_plan(plan) ? sipamd::tree_vjp::cols_per_launch(plan->g.out_len) : 0;
}

const char *sip_lqr_tree_vjp_multi_kernel_name(const sip_lqr_tree_plan *plan) {
  if (!valid_plan(plan)) // (a latched topology: no table, no kernel)
    return "";
  static const char *const names[2][sipamd::tree_vjp::kColsMax] = {
      {"tree_vjp_cols<direct,1>/f64", "tree_vjp_cols<direct,2>/f64", "tree_vjp_cols<direct,3>/f64",
       "tree_vjp_cols<direct,4>/f64", "tree_vjp_cols<direct,5>/f64", "tree_vjp_cols<direct,6>/f64",
       "tree_vjp_cols<direct,7>/f64", "tree_vjp_cols<direct,8>/f64"},
      {"tree_vjp_cols<staged,1>/f64", "tree_vjp_cols<staged,2>/f64", "tree_vjp_cols<staged,3>/f64",
       "tree_vjp_cols<staged,4>/f64", "tree_vjp_cols<staged,5>/f64", "tree_vjp_cols<staged,6>/f64",
       "tree_vjp_cols<staged,7>/f64", "tree_vjp_cols<staged,8>/f64"}};
  const int columns = sipamd::tree_vjp::cols_per_launch(plan->g.out_len);
  const sipamd::tree_vjp::ColsShape sh =
      sipamd::tree_vjp::cols_shape(plan->g.in0_len, plan->g.out_len, (long)plan->batch, columns);
  return names[sh.at.staged ? 1 : 0][columns - 1];
}

int sip_lqr_tree_vjp_input_multi(const sip_lqr_tree_plan *plan, const double *d_out_cols, const double *d_adj_cols,
                                 int num_rhs, const int32_t *d_status, double *d_grad_input, void *stream) {
  if (!valid_plan(plan) || num_rhs < 0 || d_grad_input == nullptr ||
      (num_rhs > 0 && (missing_output(plan, d_out_cols) || missing_output(plan, d_adj_cols))))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  return report(sipamd::tree_vjp::launch_tree_vjp_cols(tree_vjp_args(plan, d_out_cols, d_adj_cols, d_status, d_grad_input),
                                                       num_rhs, dev.s),
                "sip_lqr_tree_vjp_input_multi");
}

size_t sip_lqr_tree_vjp_multi_scratch_bytes(const sip_lqr_tree_plan *plan, int num_rhs) {
  return sip_lqr_tree_solve_multi_scratch_bytes(plan, num_rhs);
}

int sip_lqr_tree_vjp_multi(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work,
                           const double *d_out_cols, const double *d_grad_out_cols, int num_rhs,
                           const int32_t *d_status, double *d_adj_cols, double *d_grad_input, void *d_scratch,
                           void *stream) {
  if (!valid_plan(plan) || num_rhs < 0 || d_status == nullptr || d_work == nullptr || d_scratch == nullptr ||
      missing_input(plan, d_input) ||
      (num_rhs > 0 && (missing_output(plan, d_grad_out_cols) || missing_output(plan, d_adj_cols) ||
                       (d_grad_input != nullptr && missing_output(plan, d_out_cols)))))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  // lambda_c: K lambda_c + g_c = 0 is the plan's solve_multi with the g columns as the right-hand sides
  if (num_rhs > 0) {
    const int rc = sip_lqr_tree_solve_multi(plan, d_input, d_work, d_grad_out_cols, d_adj_cols, num_rhs, d_status,
                                            d_scratch, stream);
    if (rc != SIP_LQR_OK)
      return rc;
  }
  OnPlanDevice dev(plan, stream);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  hipError_t e = hipSuccess;
  if (num_rhs > 0 && plan->g.out_len > 0) // the solve leaves a failed problem untouched, in every column
    e = sipamd::vjp::launch_mask_cols(num_rhs, (long)plan->batch, plan->g.out_len, false, d_status, d_adj_cols, dev.s);
  if (e == hipSuccess && d_grad_input != nullptr)
    e = sipamd::tree_vjp::launch_tree_vjp_cols(tree_vjp_args(plan, d_out_cols, d_adj_cols, d_status, d_grad_input),
                                               num_rhs, dev.s);
  return report(e, "sip_lqr_tree_vjp_multi");
}

} // extern "C"
