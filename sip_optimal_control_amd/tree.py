"""General tree / variable-dimension LQR on the GPU (plumbing over the C ABI).

Mirrors the reference's `LQR` life cycle (lqr.hpp:189-194) for `batch`
instances of one topology: construct (topology compiled and latched), then
`factor()` -> statuses, `solve()` -> x, u, y, any number of times.
"""
import ctypes

import numpy as np
import torch

from ._lib import LQRLibraryError, load_library, resolve_device
from .chain import _check

_NODE_IN = ("Q", "q", "c", "delta")
_EDGE_IN = ("A", "B", "M", "R", "r")


def _ints(values):
    return (ctypes.c_int * max(1, len(values)))(*[int(v) for v in values])


def compile_topology(num_edges, root, parents, children):
    """Product-side host restatement of compile_topology_data (lqr.cpp:563-631).
    Returns (status, dict of arrays)."""
    lib = load_library()
    E, N = num_edges, num_edges + 1
    co, ce, po, cho = _ints([0] * (N + 1)), _ints([0] * E), _ints([0] * E), _ints([0] * E)
    pre, post, marks = _ints([0] * N), _ints([0] * N), _ints([0] * N)
    st = lib.sip_lqr_compile_topology(E, root, _ints(parents) if parents is not None else None,
                                      _ints(children) if children is not None else None,
                                      co, ce, po, cho, pre, post, marks)
    return st, {"child_offsets": list(co)[:N + 1], "child_edges": list(ce)[:E],
                "preorder_nodes": list(pre)[:N], "postorder_nodes": list(post)[:N]}


class BatchedTreeLQR:
    def __init__(self, parents, children, state_dims, control_dims, batch=1, root=0, device="cuda:0"):
        self._lib = load_library()
        self.E = len(control_dims)
        self.N = self.E + 1
        self.parents, self.children = list(parents), list(children)
        self.state_dims, self.control_dims = list(state_dims), list(control_dims)
        self.batch = int(batch)
        self.device = resolve_device(device)  # explicit ordinal; raises without a HIP device
        h = ctypes.c_void_p()
        _check(self._lib.sip_lqr_tree_plan_create(self.batch, self.E, root, _ints(self.parents),
                                                  _ints(self.children), _ints(self.state_dims),
                                                  _ints(self.control_dims), self.device.index,
                                                  ctypes.byref(h)), "sip_lqr_tree_plan_create")
        self._plan = h
        self.topology_status = self._lib.sip_lqr_tree_topology_status(h)
        self.in_len = self._lib.sip_lqr_tree_input_len(h)
        self.ws_len = self._lib.sip_lqr_tree_work_len(h)
        self.out_len = self._lib.sip_lqr_tree_output_len(h)
        f64 = torch.float64
        self.input = torch.zeros(self.batch, max(1, self.in_len), dtype=f64, device=self.device)
        self.work = torch.zeros(self.batch, max(1, self.ws_len), dtype=f64, device=self.device)
        self.output = torch.zeros(self.batch, max(1, self.out_len), dtype=f64, device=self.device)
        self.status = torch.full((self.batch,), -1, dtype=torch.int32, device=self.device)
        # bumped by pack() and by every factor* call: what autograd.tree_lqr_solve remembers of the factor state
        self.factor_generation = 0

    def offset(self, arena, kind, index):
        off = self._lib.sip_lqr_tree_offset(self._plan, arena, kind, index)
        if off == ctypes.c_size_t(-1).value:
            raise IndexError((arena, kind, index))
        return off

    def pack(self, problems):
        """problems: list (len batch) of blocks dicts (numpy (row, col) arrays) -> device input arena."""
        host = np.zeros((self.batch, max(1, self.in_len)))
        for b, blocks in enumerate(problems):
            for node in range(self.N):
                o = self.offset(0, 0, node)
                for name in _NODE_IN:
                    a = np.asarray(blocks[name][node], dtype=np.float64).reshape(-1, order="F")
                    host[b, o:o + a.size] = a
                    o += a.size
            for e in range(self.E):
                o = self.offset(0, 1, e)
                for name in _EDGE_IN:
                    a = np.asarray(blocks[name][e], dtype=np.float64).reshape(-1, order="F")
                    host[b, o:o + a.size] = a
                    o += a.size
        self.input.copy_(torch.from_numpy(host))
        self.factor_generation += 1

    def factor(self):
        self.factor_generation += 1
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_factor(self._plan, ctypes.c_void_p(self.input.data_ptr()),
                                             ctypes.c_void_p(self.work.data_ptr()),
                                             ctypes.c_void_p(self.status.data_ptr()),
                                             ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_factor")
        return self.status

    @property
    def kernel_name(self):
        return self._lib.sip_lqr_tree_kernel_name(self._plan).decode()

    def factor_solve(self, workspace=False):
        """factor_with_status() + solve() as one fused sweep (size-class kernel of csrc/tree_qw16.hpp
        where the tree fits one, the general engine otherwise): output, status, K and k of `work`;
        workspace=True: every LQR::Workspace field of `work` (sip_lqr_tree_factor_solve_workspace)."""
        self.factor_generation += 1
        s = torch.cuda.current_stream(self.device)
        entry = self._lib.sip_lqr_tree_factor_solve_workspace if workspace else self._lib.sip_lqr_tree_factor_solve
        scratch = self._fused_scratch()
        _check(entry(self._plan, ctypes.c_void_p(self.input.data_ptr()),
                     ctypes.c_void_p(self.work.data_ptr()),
                     ctypes.c_void_p(self.output.data_ptr()),
                     ctypes.c_void_p(self.status.data_ptr()),
                     scratch,
                     ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_factor_solve")
        return self.output, self.status

    def _fused_scratch(self):
        need = self._lib.sip_lqr_tree_fused_scratch_bytes(self._plan)
        if getattr(self, "_scratch", None) is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        return ctypes.c_void_p(self._scratch.data_ptr())

    @property
    def split_kernel_name(self):
        return self._lib.sip_lqr_tree_split_kernel_name(self._plan).decode()

    def factor_fused(self):
        """factor_with_status() alone on the size-class kernel (sip_lqr_tree_factor_fused): the factor state of
        sip_lqr_tree_factor in `work`, statuses; q, r, c are not read and `output` is not written."""
        self.factor_generation += 1
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_factor_fused(self._plan, ctypes.c_void_p(self.input.data_ptr()),
                                                   ctypes.c_void_p(self.work.data_ptr()),
                                                   ctypes.c_void_p(self.status.data_ptr()), self._fused_scratch(),
                                                   ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_factor_fused")
        return self.status

    def solve_fused(self):
        """solve() on the size-class kernel (sip_lqr_tree_solve_fused) against the factor state in `work`: x, u, y
        to `output`, v and k to `work`; problems whose status != 0 are skipped."""
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_solve_fused(self._plan, ctypes.c_void_p(self.input.data_ptr()),
                                                  ctypes.c_void_p(self.work.data_ptr()),
                                                  ctypes.c_void_p(self.output.data_ptr()),
                                                  ctypes.c_void_p(self.status.data_ptr()), self._fused_scratch(),
                                                  ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_solve_fused")
        return self.output

    def solve(self):
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_solve(self._plan, ctypes.c_void_p(self.input.data_ptr()),
                                            ctypes.c_void_p(self.work.data_ptr()),
                                            ctypes.c_void_p(self.output.data_ptr()),
                                            ctypes.c_void_p(self.status.data_ptr()),
                                            ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_solve")
        return self.output

    @property
    def multi_kernel_name(self):
        return self._lib.sip_lqr_tree_multi_kernel_name(self._plan).decode()

    @property
    def rhs_len(self):
        return self._lib.sip_lqr_tree_rhs_len(self._plan)

    def pack_rhs(self, columns):
        """columns: list (num_rhs) of lists (batch) of dicts with per-node "q", "c" and per-edge "r" (the keys
        pack() takes) -> device tensor (num_rhs, batch, rhs_len) in the layout of sip_lqr_tree_solve_multi."""
        L = self.rhs_len
        host = np.zeros((len(columns), self.batch, max(1, L)))
        for col, problems in enumerate(columns):
            for b, blocks in enumerate(problems):
                for node, n in enumerate(self.state_dims):
                    o = self._lib.sip_lqr_tree_rhs_offset(self._plan, 0, node)
                    host[col, b, o:o + n] = np.asarray(blocks["q"][node], dtype=np.float64).reshape(-1)
                    host[col, b, o + n:o + 2 * n] = np.asarray(blocks["c"][node], dtype=np.float64).reshape(-1)
                for e, m in enumerate(self.control_dims):
                    o = self._lib.sip_lqr_tree_rhs_offset(self._plan, 1, e)
                    host[col, b, o:o + m] = np.asarray(blocks["r"][e], dtype=np.float64).reshape(-1)
        return torch.from_numpy(host).to(self.device)

    def solve_multi(self, rhs_cols, out_cols=None):
        """LQR::solve for several right-hand sides against the factor state in `work` (left by factor() or
        factor_solve(workspace=True)); rhs_cols: (num_rhs, batch, rhs_len) float64 on the device (pack_rhs).
        Returns the output columns (num_rhs, batch, output_len); problems whose status != 0 keep what
        out_cols held."""
        rhs_cols = rhs_cols.contiguous()
        num_rhs = rhs_cols.shape[0]
        if out_cols is None:
            out_cols = torch.zeros(num_rhs, self.batch, max(1, self.out_len), dtype=torch.float64, device=self.device)
        need = self._lib.sip_lqr_tree_solve_multi_scratch_bytes(self._plan, num_rhs)
        if getattr(self, "_multi_scratch", None) is None or self._multi_scratch.numel() < need:
            self._multi_scratch = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_solve_multi(self._plan, ctypes.c_void_p(self.input.data_ptr()),
                                                  ctypes.c_void_p(self.work.data_ptr()),
                                                  ctypes.c_void_p(rhs_cols.data_ptr()),
                                                  ctypes.c_void_p(out_cols.data_ptr()), num_rhs,
                                                  ctypes.c_void_p(self.status.data_ptr()),
                                                  ctypes.c_void_p(self._multi_scratch.data_ptr()),
                                                  ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_solve_multi")
        return out_cols

    @property
    def residual_kernel_name(self):
        return self._lib.sip_lqr_tree_residual_kernel_name(self._plan).decode()

    def _rhs_ptr(self, rhs):
        """One column of right-hand sides (batch, rhs_len) float64 on the device, or None: q, c, r of `input`."""
        if rhs is None:
            return None
        if rhs.dtype != torch.float64 or not rhs.is_contiguous() or rhs.numel() != self.batch * max(1, self.rhs_len):
            raise ValueError("rhs: contiguous torch.float64 of (batch, rhs_len)")
        return ctypes.c_void_p(rhs.data_ptr())

    def residual(self, output=None, rhs=None, want_vector=True):
        """The residual of the KKT system at `output` (default: self.output), in fp64 (sip_lqr_tree_residual):
        (res [batch, rhs_len] in the layout of a right-hand side of solve_multi, or None with want_vector=False;
        norm [batch] = max |res| per problem).  rhs: one column (batch, rhs_len) in place of q, c, r of `input`."""
        output = self.output if output is None else output
        res = torch.empty(self.batch, max(1, self.rhs_len), dtype=torch.float64, device=self.device) \
            if want_vector else None
        norm = torch.empty(self.batch, dtype=torch.float64, device=self.device)
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_residual(self._plan, ctypes.c_void_p(self.input.data_ptr()), self._rhs_ptr(rhs),
                                               ctypes.c_void_p(output.data_ptr()),
                                               ctypes.c_void_p(res.data_ptr() if want_vector else None),
                                               ctypes.c_void_p(norm.data_ptr()),
                                               ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_residual")
        return res, norm

    def refine(self, iterations=2, rhs=None, output=None):
        """Iterative refinement in fp64 around the plan's solve, against the factor state in `work` (left by factor(),
        factor_fused() or factor_solve(workspace=True)) (sip_lqr_tree_refine): `iterations` rounds of residual ->
        one-column solve -> update, then one more residual.  output: the starting iterate (batch, output_len),
        refined in place, or None: from zero into self.output (round 1 is then the plain solve).  Problems whose
        status is not SUCCESS keep their iterate.  Returns (output, norms [iterations + 1, batch]): norms[j] before
        round j + 1, norms[-1] of the result."""
        from_zero = output is None
        if from_zero:
            output = self.output
        if output.dtype != torch.float64 or not output.is_contiguous():
            raise ValueError("output: contiguous torch.float64")
        norms = torch.empty(int(iterations) + 1, self.batch, dtype=torch.float64, device=self.device)
        need = self._lib.sip_lqr_tree_refine_workspace_bytes(self._plan)
        if getattr(self, "_refine_scratch", None) is None or self._refine_scratch.numel() < need:
            self._refine_scratch = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_refine(self._plan, ctypes.c_void_p(self.input.data_ptr()),
                                             ctypes.c_void_p(self.work.data_ptr()), self._rhs_ptr(rhs),
                                             ctypes.c_void_p(output.data_ptr()), int(iterations),
                                             1 if from_zero else 0, ctypes.c_void_p(self.status.data_ptr()),
                                             ctypes.c_void_p(self._refine_scratch.data_ptr()),
                                             ctypes.c_void_p(norms.data_ptr()),
                                             ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_refine")
        return output, norms

    @property
    def residual_multi_kernel_name(self):
        return self._lib.sip_lqr_tree_residual_multi_kernel_name(self._plan).decode()

    @property
    def residual_multi_columns(self):
        """Columns one launch of residual_multi carries on this plan (sip_lqr_tree_residual_multi_columns)."""
        return int(self._lib.sip_lqr_tree_residual_multi_columns(self._plan))

    def _cols(self, t, name):
        """num_rhs of a contiguous float64 [num_rhs, batch, rhs_len] column array on the plan's device."""
        if t.dtype != torch.float64 or t.device != self.device or not t.is_contiguous() or t.dim() != 3 \
                or tuple(t.shape[1:]) != (self.batch, max(1, self.rhs_len)):
            raise ValueError(f"{name}: expected contiguous torch.float64 "
                             f"[num_rhs, {self.batch}, {max(1, self.rhs_len)}] on {self.device}")
        return int(t.shape[0])

    def residual_multi(self, out_cols, rhs_cols=None, want_vector=True):
        """residual() for several iterates and right-hand sides against one `input` (sip_lqr_tree_residual_multi):
        out_cols (num_rhs, batch, output_len) as solve_multi returns them; rhs_cols likewise (pack_rhs), or None: q, c, r
        of `input` for every column.  Returns (res_cols [num_rhs, batch, rhs_len], or None with want_vector=False;
        norms [num_rhs, batch]).  Column c is bit for bit residual(out_cols[c], rhs=rhs_cols[c])."""
        num_rhs = self._cols(out_cols, "out_cols")
        if rhs_cols is not None and self._cols(rhs_cols, "rhs_cols") != num_rhs:
            raise ValueError("rhs_cols: as many columns as out_cols")
        res = torch.empty(num_rhs, self.batch, max(1, self.rhs_len), dtype=torch.float64, device=self.device) \
            if want_vector else None
        norms = torch.empty(num_rhs, self.batch, dtype=torch.float64, device=self.device)
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_residual_multi(
            self._plan, ctypes.c_void_p(self.input.data_ptr()),
            ctypes.c_void_p(rhs_cols.data_ptr() if rhs_cols is not None else None),
            ctypes.c_void_p(out_cols.data_ptr()), num_rhs, ctypes.c_void_p(res.data_ptr() if want_vector else None),
            ctypes.c_void_p(norms.data_ptr()), ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_residual_multi")
        return res, norms

    def refine_multi(self, rhs_cols, iterations=2, out_cols=None):
        """refine() for several right-hand sides around solve_multi(), against the factor state in `work`
        (sip_lqr_tree_refine_multi): rhs_cols (num_rhs, batch, rhs_len) (pack_rhs); out_cols the starting iterates,
        refined in place, or None: from zero (round 1 is then the plain solve_multi).  A problem whose status is not
        SUCCESS keeps its iterate in every column.  Returns (out_cols, norms [iterations + 1, num_rhs, batch])."""
        num_rhs = self._cols(rhs_cols, "rhs_cols")
        from_zero = out_cols is None
        if from_zero:
            out_cols = torch.empty(num_rhs, self.batch, max(1, self.out_len), dtype=torch.float64, device=self.device)
        if self._cols(out_cols, "out_cols") != num_rhs:
            raise ValueError("out_cols: as many columns as rhs_cols")
        norms = torch.empty(int(iterations) + 1, num_rhs, self.batch, dtype=torch.float64, device=self.device)
        need = self._lib.sip_lqr_tree_refine_multi_workspace_bytes(self._plan, num_rhs)
        if getattr(self, "_refine_multi_scratch", None) is None or self._refine_multi_scratch.numel() < need:
            self._refine_multi_scratch = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_refine_multi(
            self._plan, ctypes.c_void_p(self.input.data_ptr()), ctypes.c_void_p(self.work.data_ptr()),
            ctypes.c_void_p(rhs_cols.data_ptr()), ctypes.c_void_p(out_cols.data_ptr()), num_rhs, int(iterations),
            1 if from_zero else 0, ctypes.c_void_p(self.status.data_ptr()),
            ctypes.c_void_p(self._refine_multi_scratch.data_ptr()), ctypes.c_void_p(norms.data_ptr()),
            ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_refine_multi")
        return out_cols, norms

    @property
    def vjp_kernel_name(self):
        return self._lib.sip_lqr_tree_vjp_kernel_name(self._plan).decode()

    def _arena(self, t, length, name):
        if t.dtype != torch.float64 or t.device != self.device or not t.is_contiguous() \
                or t.numel() != self.batch * max(1, length):
            raise ValueError(f"{name}: expected contiguous torch.float64 [{self.batch}, {max(1, length)}] on {self.device}")
        return ctypes.c_void_p(t.data_ptr())

    def vjp_input(self, output, adj, use_status=True, grad_input=None):
        """The gradient kernel alone (sip_lqr_tree_vjp_input): grad_input [batch, in_len] in the input arena's layout
        (written to `grad_input` when given) from output (z) and adj (lambda), both [batch, output_len]; use_status:
        problems whose status != 0 get zeros."""
        grad = grad_input if grad_input is not None else \
            torch.empty(self.batch, max(1, self.in_len), dtype=torch.float64, device=self.device)
        self._arena(grad, self.in_len, "grad_input")
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_vjp_input(self._plan, self._arena(output, self.out_len, "output"),
                                                self._arena(adj, self.out_len, "adj"),
                                                ctypes.c_void_p(self.status.data_ptr() if use_status else None),
                                                ctypes.c_void_p(grad.data_ptr()), ctypes.c_void_p(s.cuda_stream)),
               "sip_lqr_tree_vjp_input")
        return grad

    def vjp(self, grad_output, output=None, want_input=True, refine_iterations=0):
        """The backward pass of the solve for a loss with dL/d(output) = grad_output [batch, output_len], against the
        factor state in `work` (left by factor(), factor_fused() or factor_solve(workspace=True)) (sip_lqr_tree_vjp):
        one adjoint solve, K adj + grad_output = 0, then the outer-product kernel on `output` (default: self.output)
        and adj.  Returns (grad_input [batch, in_len] in the input arena's layout, or None with want_input=False;
        adj [batch, output_len] = dL/d(q, c, r) in the layout of a right-hand side).  refine_iterations > 0: adj comes
        from that many rounds of refine() on grad_output instead of the plain solve.  Problems whose status != 0 get
        zeros in both.  The gains are not differentiated."""
        output = self.output if output is None else output
        g = self._arena(grad_output, self.out_len, "grad_output")
        if want_input:
            self._arena(output, self.out_len, "output")
        if int(refine_iterations) > 0:
            adj = torch.zeros(self.batch, max(1, self.out_len), dtype=torch.float64, device=self.device)
            self.refine(iterations=int(refine_iterations), rhs=grad_output, output=adj)
            adj.masked_fill_((self.status != 0).unsqueeze(1), 0.0)
            return (self.vjp_input(output, adj) if want_input else None), adj
        adj = torch.empty(self.batch, max(1, self.out_len), dtype=torch.float64, device=self.device)
        grad = torch.empty(self.batch, max(1, self.in_len), dtype=torch.float64, device=self.device) \
            if want_input else None
        need = self._lib.sip_lqr_tree_vjp_scratch_bytes(self._plan)
        if getattr(self, "_multi_scratch", None) is None or self._multi_scratch.numel() < need:
            self._multi_scratch = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_vjp(self._plan, ctypes.c_void_p(self.input.data_ptr()),
                                          ctypes.c_void_p(self.work.data_ptr()), ctypes.c_void_p(output.data_ptr()), g,
                                          ctypes.c_void_p(self.status.data_ptr()), ctypes.c_void_p(adj.data_ptr()),
                                          ctypes.c_void_p(grad.data_ptr() if want_input else None),
                                          ctypes.c_void_p(self._multi_scratch.data_ptr()),
                                          ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_vjp")
        return grad, adj

    @property
    def vjp_multi_columns(self):
        """Columns one launch of the multi-column gradient kernel carries on this plan
        (sip_lqr_tree_vjp_multi_columns)."""
        return int(self._lib.sip_lqr_tree_vjp_multi_columns(self._plan))

    @property
    def vjp_multi_kernel_name(self):
        return self._lib.sip_lqr_tree_vjp_multi_kernel_name(self._plan).decode()

    def vjp_input_multi(self, out_cols, adj_cols, use_status=True, grad_input=None):
        """The multi-column gradient kernel alone (sip_lqr_tree_vjp_input_multi): ONE grad_input [batch, in_len] in the
        input arena's layout (written to `grad_input` when given), the sum over the columns of out_cols (z_c) and
        adj_cols (lambda_c), both [num_rhs, batch, output_len]; the q, c, r slots are +0.0 (solve_multi does not read
        them: their gradient is adj_cols).  No column: zeros.  use_status: problems whose status != 0 get zeros."""
        num_rhs = self._cols(out_cols, "out_cols")
        if self._cols(adj_cols, "adj_cols") != num_rhs:
            raise ValueError("adj_cols: as many columns as out_cols")
        grad = grad_input if grad_input is not None else \
            torch.empty(self.batch, max(1, self.in_len), dtype=torch.float64, device=self.device)
        self._arena(grad, self.in_len, "grad_input")
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_vjp_input_multi(
            self._plan, ctypes.c_void_p(out_cols.data_ptr()), ctypes.c_void_p(adj_cols.data_ptr()), num_rhs,
            ctypes.c_void_p(self.status.data_ptr() if use_status else None), ctypes.c_void_p(grad.data_ptr()),
            ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_vjp_input_multi")
        return grad

    def vjp_multi(self, grad_out_cols, out_cols, want_input=True, refine_iterations=0):
        """The backward pass of solve_multi for a loss with dL/d(out_cols) = grad_out_cols [num_rhs, batch,
        output_len], against the factor state in `work` (sip_lqr_tree_vjp_multi): one adjoint solve_multi,
        K adj_c + grad_out_c = 0, then the multi-column kernel on out_cols and adj_cols.  Returns (grad_input [batch,
        in_len], summed over the columns, +0.0 in the q, c, r slots, or None with want_input=False; adj_cols [num_rhs,
        batch, output_len] = dL/d(rhs_cols)).  refine_iterations > 0: adj_cols comes from that many rounds of
        refine_multi() on grad_out_cols from a zero iterate instead of the plain solve.  Problems whose status != 0
        get zeros in both.  The gains are not differentiated."""
        num_rhs = self._cols(grad_out_cols, "grad_out_cols")
        if want_input and self._cols(out_cols, "out_cols") != num_rhs:
            raise ValueError("out_cols: as many columns as grad_out_cols")
        if int(refine_iterations) > 0:
            adj = torch.zeros(num_rhs, self.batch, max(1, self.out_len), dtype=torch.float64, device=self.device)
            self.refine_multi(grad_out_cols, iterations=int(refine_iterations), out_cols=adj)
            adj.masked_fill_((self.status != 0).reshape(1, -1, 1), 0.0)
            return (self.vjp_input_multi(out_cols, adj) if want_input else None), adj
        adj = torch.empty(num_rhs, self.batch, max(1, self.out_len), dtype=torch.float64, device=self.device)
        grad = torch.empty(self.batch, max(1, self.in_len), dtype=torch.float64, device=self.device) \
            if want_input else None
        need = self._lib.sip_lqr_tree_vjp_multi_scratch_bytes(self._plan, num_rhs)
        if getattr(self, "_multi_scratch", None) is None or self._multi_scratch.numel() < need:
            self._multi_scratch = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        s = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_tree_vjp_multi(
            self._plan, ctypes.c_void_p(self.input.data_ptr()), ctypes.c_void_p(self.work.data_ptr()),
            ctypes.c_void_p(out_cols.data_ptr() if want_input else None), ctypes.c_void_p(grad_out_cols.data_ptr()),
            num_rhs, ctypes.c_void_p(self.status.data_ptr()), ctypes.c_void_p(adj.data_ptr()),
            ctypes.c_void_p(grad.data_ptr() if want_input else None), ctypes.c_void_p(self._multi_scratch.data_ptr()),
            ctypes.c_void_p(s.cuda_stream)), "sip_lqr_tree_vjp_multi")
        return grad, adj

    def unpack_solution(self, b=0, output=None):
        out = (self.output[b] if output is None else output[b]).cpu().numpy()
        x, y, u = [], [], []
        for node, n in enumerate(self.state_dims):
            o = self.offset(2, 0, node)
            x.append(out[o:o + n].copy())
            y.append(out[o + n:o + 2 * n].copy())
        for e, m in enumerate(self.control_dims):
            o = self.offset(2, 1, e)
            u.append(out[o:o + m].copy())
        return x, u, y

    def unpack_gains(self, b=0):
        ws = self.work[b].cpu().numpy()
        max_n = max(self.state_dims) if self.state_dims else 0
        Ks, ks = [], []
        for e, m in enumerate(self.control_dims):
            n = self.state_dims[self.parents[e]]
            o = self.offset(1, 1, e) + max_n * max_n
            Ks.append(ws[o:o + m * n].reshape((m, n), order="F").copy())
            o += m * n + m * m
            ks.append(ws[o:o + m].copy())
        return Ks, ks

    def topology_arrays(self):
        names = ["child_offsets", "child_edges", "preorder_nodes", "postorder_nodes"]
        sizes = [self.N + 1, self.E, self.N, self.N]
        out = {}
        for which, (name, size) in enumerate(zip(names, sizes)):
            ptr = self._lib.sip_lqr_tree_topology_array(self._plan, which)
            out[name] = [ptr[i] for i in range(size)]
        return out

    def close(self):
        if getattr(self, "_plan", None):
            self._lib.sip_lqr_tree_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
