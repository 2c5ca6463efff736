"""Batched uniform-chain LQR on the GPU: thin torch/ctypes plumbing over the C ABI.

Mirrors the reference's `LQR` object life cycle (sip_optimal_control/lqr.hpp:
189-194): construct once per shape (topology compiled once), then
`factor_solve()` (= factor_with_status() + solve()) as often as needed on
device-resident packed buffers.  No arithmetic happens in Python.
"""
import ctypes
import enum

import torch

from ._lib import LQRLibraryError, load_library, resolve_device
from .layout import ChainShape


class FactorStatus(enum.IntEnum):
    """sip_optimal_control/lqr.hpp:68-74."""
    SUCCESS = 0
    INVALID_DELTA = 1
    F_FACTORIZATION_FAILURE = 2
    G_FACTORIZATION_FAILURE = 3
    INVALID_TOPOLOGY = 4


_DTYPES = {torch.float64: 0, torch.float32: 1}


def _check(code, what):
    if code != 0:
        names = {-1: "invalid argument", -2: "unsupported shape/dtype (no HIP kernel)",
                 -3: "HIP runtime error", -4: "allocation failure"}
        raise LQRLibraryError(f"{what} failed: {names.get(code, code)}")


class BatchedChainLQR:
    """`batch` independent chain problems of horizon T, state dim n, control dim m."""

    def __init__(self, n, m, T, batch, dtype=torch.float64, device="cuda:0", symmetric=False, separate_sweeps=False,
                 fused_f32=False, wide_controls=False):
        """wide_controls=True: a plan of the general engine with 9 <= m <= 16 controls and n <= 32 runs on the n = 32
        matrix-core kernel for 12 or 16 controls: n = 32 with m in {12, 16} on the exact kernel in either dtype, every
        other fp64 shape embedded in the one with the least M >= m (sip_lqr_plan_set_wide_controls; a no-op on other
        plans, see `has_wide_controls`).  Applied before separate_sweeps, which these rows take like the m <= 8 ones.
        fused_f32=True: an fp32 plan whose (n, m) has a fused fp32 kernel (n <= 15, m <= 8: the benchmark grid
        n in {4, 6, 8, 12} x m in {1, 2, 3, 4} and a few more) runs on it instead of the general engine
        (sip_lqr_plan_set_fused_f32; a no-op on other plans, see `has_fused_f32`).
        separate_sweeps=True: on plans of the n = 32 matrix-core kernel (16 < n <= 32, m <= 8) and on plans on which
        fused_f32 took effect (it is applied first), factor() runs the matrix sweep alone, solve() a vector-only
        sweep against it and solve_multi() up to 16 (n = 32) or 8 (fused fp32) columns per sweep
        (sip_lqr_plan_set_separate_sweeps; a no-op on other plans, see `has_separate_sweeps`).
        symmetric=True: `mats` in SIP_LQR_LAYOUT_SYMMETRIC (Q, R as packed lower triangles; ChainShape.pack_index
        converts a full-layout batch); raises for shapes without a symmetric-packed kernel."""
        self._lib = load_library()
        self.shape = ChainShape(n, m, T, symmetric=bool(symmetric))
        self.batch = int(batch)
        self.dtype = dtype
        self.device = resolve_device(device)  # explicit ordinal; raises without a HIP device
        handle = ctypes.c_void_p()
        _check(self._lib.sip_lqr_plan_create_layout(_DTYPES[dtype], self.batch, T, n, m, self.device.index,
                                                    1 if symmetric else 0, ctypes.byref(handle)),
               f"sip_lqr_plan_create_layout(n={n}, m={m}, T={T}, {dtype}, symmetric={bool(symmetric)})")
        self._plan = handle
        if fused_f32:  # before any size is read
            _check(self._lib.sip_lqr_plan_set_fused_f32(handle, 1), "sip_lqr_plan_set_fused_f32")
        if wide_controls:  # likewise
            _check(self._lib.sip_lqr_plan_set_wide_controls(handle, 1), "sip_lqr_plan_set_wide_controls")
        if separate_sweeps:  # likewise; after fused_f32 and wide_controls: their rows have separate sweeps to opt into
            _check(self._lib.sip_lqr_plan_set_separate_sweeps(handle, 1), "sip_lqr_plan_set_separate_sweeps")
        esize = torch.empty((), dtype=dtype).element_size()
        assert self._lib.sip_lqr_mats_len(handle) == self.shape.mats_len
        assert self._lib.sip_lqr_vecs_len(handle) == self.shape.vecs_len
        assert self._lib.sip_lqr_gains_len(handle) == self.shape.gains_len
        ws_elems = -(-self._lib.sip_lqr_workspace_bytes(handle) // esize)
        self.workspace = torch.empty(ws_elems, dtype=dtype, device=self.device)
        self.status = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        # bumped by every factor* call: what a saved backward pass compares to know whether the factor state in the
        # workspace is still its own (autograd.chain_lqr_solve)
        self.factor_generation = 0

    @property
    def kernel_name(self):
        return self._lib.sip_lqr_kernel_name(self._plan).decode()

    @property
    def has_separate_sweeps(self):
        """True when the separate_sweeps opt-in took effect on this plan."""
        return bool(self._lib.sip_lqr_has_separate_sweeps(self._plan))

    @property
    def has_fused_f32(self):
        """True when the fused_f32 opt-in took effect on this plan."""
        return bool(self._lib.sip_lqr_has_fused_f32(self._plan))

    @property
    def has_wide_controls(self):
        """True when the wide_controls opt-in took effect on this plan."""
        return bool(self._lib.sip_lqr_has_wide_controls(self._plan))

    def empty_sol(self):
        return torch.empty(self.batch, self.shape.vecs_len, dtype=self.dtype, device=self.device)

    def empty_gains(self):
        return torch.empty(self.batch, self.shape.gains_len, dtype=self.dtype, device=self.device)

    def _ptr(self, t, rows, cols, name):
        if t.dtype != self.dtype or t.device != self.device or not t.is_contiguous() \
                or t.numel() != rows * cols:
            raise ValueError(f"{name}: expected contiguous {self.dtype} [{rows}, {cols}] on {self.device}")
        return ctypes.c_void_p(t.data_ptr())

    def factor_solve(self, mats, vecs, sol=None, gains=None, stream=None):
        """One fused Riccati sweep (factor + solve) over the whole batch.

        Asynchronous on `stream` (default: torch's current stream).  Returns
        (sol, gains, status) device tensors in the packed chain layout.
        """
        s = self.shape
        if sol is None:
            sol = self.empty_sol()
        if gains is None:
            gains = self.empty_gains()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        self.factor_generation += 1
        _check(self._lib.sip_lqr_factor_solve(
            self._plan, self._ptr(mats, self.batch, s.mats_len, "mats"),
            self._ptr(vecs, self.batch, s.vecs_len, "vecs"),
            self._ptr(sol, self.batch, s.vecs_len, "sol"),
            self._ptr(gains, self.batch, s.gains_len, "gains"),
            ctypes.c_void_p(self.status.data_ptr()),
            ctypes.c_void_p(self.workspace.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_factor_solve")
        return sol, gains, self.status

    @property
    def has_split(self):
        """True when sip_lqr_factor_solve_split serves this plan (A | B read in place)."""
        return bool(self._lib.sip_lqr_has_split(self._plan))

    def split_inputs(self, mats):
        """The inputs of factor_solve_split cut out of packed `mats` [batch, mats_len]: (qmr, ab) with
        qmr [batch, split_mats_len] = node blocks [Q | delta], edge blocks [M | R], and ab [batch, T, n * (n + m)]
        = A | B per stage.  A test / demo helper: callers of the split entry point have A | B elsewhere already."""
        s = self.shape
        n, m, T = s.n, s.m, s.T
        node, edge, abn = s.node, s.edge, n * n + n * m  # (Q, R packed triangles in the symmetric layout)
        stg = node + edge
        body = mats[:, :T * stg].reshape(self.batch, T, stg)
        qmr = torch.cat([torch.cat([body[:, :, :node], body[:, :, node + abn:]], dim=2).reshape(self.batch, -1),
                         mats[:, T * stg:]], dim=1).contiguous()
        assert qmr.shape[1] == int(self._lib.sip_lqr_split_mats_len(self._plan))
        return qmr, body[:, :, node:node + abn].contiguous()

    def factor_solve_split(self, qmr, ab, vecs, sol=None, gains=None, stream=None):
        """factor_solve with the dynamics Jacobians read in place (sip_lqr_factor_solve_split): `ab` any
        tensor whose element [p, i] holds A | B of stage i (strides taken from the tensor)."""
        s = self.shape
        if sol is None:
            sol = self.empty_sol()
        if gains is None:
            gains = self.empty_gains()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        assert ab.dtype == torch.float64 and ab.stride(-1) == 1 and ab.shape[-1] >= s.n * (s.n + s.m)
        self.factor_generation += 1
        _check(self._lib.sip_lqr_factor_solve_split(
            self._plan, ctypes.c_void_p(qmr.data_ptr()), ctypes.c_void_p(ab.data_ptr()),
            ctypes.c_int64(ab.stride(0)), ctypes.c_int64(ab.stride(1) if ab.dim() > 2 else 0),
            self._ptr(vecs, self.batch, s.vecs_len, "vecs"),
            self._ptr(sol, self.batch, s.vecs_len, "sol"),
            self._ptr(gains, self.batch, s.gains_len, "gains"),
            ctypes.c_void_p(self.status.data_ptr()),
            ctypes.c_void_p(self.workspace.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_factor_solve_split")
        return sol, gains, self.status

    def factor(self, mats, gains=None, stream=None):
        """LQR::factor_with_status() alone (the plan's fused sweep, or the general engine): statuses, K part of gains,
        factor state kept in the workspace for later solve() calls."""
        s = self.shape
        if gains is None:
            gains = self.empty_gains()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        self.factor_generation += 1
        _check(self._lib.sip_lqr_factor(
            self._plan, self._ptr(mats, self.batch, s.mats_len, "mats"),
            self._ptr(gains, self.batch, s.gains_len, "gains"),
            ctypes.c_void_p(self.status.data_ptr()), ctypes.c_void_p(self.workspace.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_factor")
        return gains, self.status

    def solve(self, mats, vecs, gains, sol=None, stream=None):
        """LQR::solve() alone against the last factor(); repeatable with new vecs."""
        s = self.shape
        if sol is None:
            sol = self.empty_sol()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_solve(
            self._plan, self._ptr(mats, self.batch, s.mats_len, "mats"),
            self._ptr(vecs, self.batch, s.vecs_len, "vecs"),
            self._ptr(sol, self.batch, s.vecs_len, "sol"),
            self._ptr(gains, self.batch, s.gains_len, "gains"),
            ctypes.c_void_p(self.workspace.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_solve")
        return sol

    def solve_multi_workspace_bytes(self, num_rhs):
        """Column workspace sip_lqr_solve_multi needs for `num_rhs` columns; 0: the shape has no multi-rhs kernel
        and the columns are solved one by one."""
        return int(self._lib.sip_lqr_solve_multi_workspace_bytes(self._plan, int(num_rhs)))

    def solve_multi(self, mats, vecs_cols, gains, sol_cols=None, stream=None):
        """LQR::solve() for several right-hand sides against the last factor() (the multi-rhs block of
        solve_stagewise_kkt_matrix, helpers.cpp:521-665): vecs_cols / sol_cols are [num_rhs, batch,
        vecs_len].  One sweep per 8 columns where the shape has the multi-rhs kernel or the plan runs the fused fp32
        kernel with separate_sweeps (per 16 on the n = 32 plans with separate_sweeps); column by column otherwise."""
        s = self.shape
        num_rhs = vecs_cols.shape[0]
        if sol_cols is None:
            sol_cols = torch.empty(num_rhs, self.batch, s.vecs_len, dtype=self.dtype, device=self.device)
        for t, name in ((vecs_cols, "vecs_cols"), (sol_cols, "sol_cols")):
            if t.dtype != self.dtype or t.device != self.device or not t.is_contiguous() or \
                    tuple(t.shape) != (num_rhs, self.batch, s.vecs_len):
                raise ValueError(f"{name}: expected contiguous {self.dtype} [{num_rhs}, {self.batch}, {s.vecs_len}]")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        need = self._lib.sip_lqr_solve_multi_workspace_bytes(self._plan, num_rhs)
        if getattr(self, "_col_ws", None) is None or self._col_ws.numel() < need:
            self._col_ws = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        _check(self._lib.sip_lqr_solve_multi(
            self._plan, self._ptr(mats, self.batch, s.mats_len, "mats"), ctypes.c_void_p(vecs_cols.data_ptr()),
            ctypes.c_void_p(sol_cols.data_ptr()), num_rhs, self._ptr(gains, self.batch, s.gains_len, "gains"),
            ctypes.c_void_p(self.workspace.data_ptr()), ctypes.c_void_p(self._col_ws.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_solve_multi")
        return sol_cols

    def _wide(self, vecs, sol):
        """0 / 1: `vecs` and `sol` are both in the plan's dtype / both float64 (sip_lqr_residual's `wide`)."""
        if vecs.dtype != sol.dtype or vecs.dtype not in (self.dtype, torch.float64):
            raise ValueError(f"vecs and sol: both {self.dtype} or both torch.float64")
        for t, name in ((vecs, "vecs"), (sol, "sol")):
            if t.device != self.device or not t.is_contiguous() or t.numel() != self.batch * self.shape.vecs_len:
                raise ValueError(f"{name}: expected contiguous [{self.batch}, {self.shape.vecs_len}] on {self.device}")
        return 1 if vecs.dtype == torch.float64 else 0

    def residual(self, mats, vecs, sol, want_vector=True, stream=None):
        """The residual of the KKT system at `sol`, in fp64 (sip_lqr_residual): (res64 [batch, vecs_len] in the vecs
        layout, or None with want_vector=False; norm [batch] = max |res| per problem).  vecs and sol: both in the
        plan's dtype or both float64."""
        s = self.shape
        wide = self._wide(vecs, sol)
        res = torch.empty(self.batch, s.vecs_len, dtype=torch.float64, device=self.device) if want_vector else None
        norm = torch.empty(self.batch, dtype=torch.float64, device=self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_residual(
            self._plan, self._ptr(mats, self.batch, s.mats_len, "mats"), ctypes.c_void_p(vecs.data_ptr()),
            ctypes.c_void_p(sol.data_ptr()), wide, ctypes.c_void_p(res.data_ptr() if want_vector else None),
            ctypes.c_void_p(norm.data_ptr()), ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_residual")
        return res, norm

    def refine(self, mats, vecs64, gains, iterations=3, sol=None, use_status=True, stream=None):
        """Iterative refinement in fp64 around solve(), against the last factor() (sip_lqr_refine): `iterations`
        rounds of residual -> solve -> update, then one more residual.  vecs64: float64 [batch, vecs_len]; sol: the
        float64 starting iterate, refined in place, or None to start from zero (round 1 is then the plain solve).
        Problems whose factor status is not SUCCESS keep their iterate (use_status=False: nothing is skipped).
        Returns (sol64, norms [iterations + 1, batch]): norms[j] before round j + 1, norms[-1] of the result."""
        s = self.shape
        from_zero = sol is None
        if from_zero:
            sol = torch.empty(self.batch, s.vecs_len, dtype=torch.float64, device=self.device)
        if vecs64.dtype != torch.float64 or self._wide(vecs64, sol) != 1:
            raise ValueError("vecs64 and sol: torch.float64")
        norms = torch.empty(int(iterations) + 1, self.batch, dtype=torch.float64, device=self.device)
        if getattr(self, "_refine_ws", None) is None:  # once per plan
            self._refine_ws = torch.empty(max(1, self._lib.sip_lqr_refine_workspace_bytes(self._plan)),
                                          dtype=torch.uint8, device=self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_refine(
            self._plan, self._ptr(mats, self.batch, s.mats_len, "mats"), ctypes.c_void_p(vecs64.data_ptr()),
            ctypes.c_void_p(sol.data_ptr()), int(iterations), 1 if from_zero else 0,
            self._ptr(gains, self.batch, s.gains_len, "gains"), ctypes.c_void_p(self.workspace.data_ptr()),
            ctypes.c_void_p(self._refine_ws.data_ptr()),
            ctypes.c_void_p(self.status.data_ptr() if use_status else None), ctypes.c_void_p(norms.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_refine")
        return sol, norms

    @property
    def residual_multi_columns(self):
        """Columns one launch of residual_multi carries on this plan (sip_lqr_residual_multi_columns)."""
        return int(self._lib.sip_lqr_residual_multi_columns(self._plan))

    def _cols(self, t, name, dtypes):
        """num_rhs of a contiguous [num_rhs, batch, vecs_len] column array on the plan's device."""
        if t.dtype not in dtypes or t.device != self.device or not t.is_contiguous() or t.dim() != 3 \
                or tuple(t.shape[1:]) != (self.batch, self.shape.vecs_len):
            raise ValueError(f"{name}: expected contiguous {' or '.join(map(str, dtypes))} "
                             f"[num_rhs, {self.batch}, {self.shape.vecs_len}] on {self.device}")
        return int(t.shape[0])

    def residual_multi(self, mats, vecs_cols, sol_cols, want_vector=True, stream=None):
        """residual() for several right-hand sides and iterates against one `mats` (sip_lqr_residual_multi):
        vecs_cols / sol_cols are [num_rhs, batch, vecs_len], both in the plan's dtype or both float64.  Returns
        (res64 [num_rhs, batch, vecs_len], or None with want_vector=False; norms [num_rhs, batch]).  Column c is bit
        for bit residual() on that column."""
        s = self.shape
        num_rhs = self._cols(vecs_cols, "vecs_cols", (self.dtype, torch.float64))
        if self._cols(sol_cols, "sol_cols", (vecs_cols.dtype,)) != num_rhs:
            raise ValueError("sol_cols: as many columns as vecs_cols")
        wide = 1 if vecs_cols.dtype == torch.float64 else 0
        res = torch.empty(num_rhs, self.batch, s.vecs_len, dtype=torch.float64, device=self.device) \
            if want_vector else None
        norms = torch.empty(num_rhs, self.batch, dtype=torch.float64, device=self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_residual_multi(
            self._plan, self._ptr(mats, self.batch, s.mats_len, "mats"), ctypes.c_void_p(vecs_cols.data_ptr()),
            ctypes.c_void_p(sol_cols.data_ptr()), num_rhs, wide,
            ctypes.c_void_p(res.data_ptr() if want_vector else None), ctypes.c_void_p(norms.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_residual_multi")
        return res, norms

    def refine_multi(self, mats, vecs64_cols, gains, iterations=3, sol_cols=None, use_status=True, stream=None):
        """refine() for several right-hand sides around solve_multi(), against the last factor()
        (sip_lqr_refine_multi): vecs64_cols float64 [num_rhs, batch, vecs_len]; sol_cols the float64 starting
        iterates, refined in place, or None to start from zero.  A problem whose factor status is not SUCCESS keeps
        its iterate in every column (use_status=False: nothing is skipped).  Returns (sol64_cols, norms
        [iterations + 1, num_rhs, batch])."""
        s = self.shape
        num_rhs = self._cols(vecs64_cols, "vecs64_cols", (torch.float64,))
        from_zero = sol_cols is None
        if from_zero:
            sol_cols = torch.empty(num_rhs, self.batch, s.vecs_len, dtype=torch.float64, device=self.device)
        if self._cols(sol_cols, "sol_cols", (torch.float64,)) != num_rhs:
            raise ValueError("sol_cols: as many columns as vecs64_cols")
        norms = torch.empty(int(iterations) + 1, num_rhs, self.batch, dtype=torch.float64, device=self.device)
        need = self._lib.sip_lqr_refine_multi_workspace_bytes(self._plan, num_rhs)
        if getattr(self, "_refine_multi_ws", None) is None or self._refine_multi_ws.numel() < need:  # grows with num_rhs
            self._refine_multi_ws = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        need = self._lib.sip_lqr_solve_multi_workspace_bytes(self._plan, num_rhs)
        if getattr(self, "_col_ws", None) is None or self._col_ws.numel() < need:
            self._col_ws = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_refine_multi(
            self._plan, self._ptr(mats, self.batch, s.mats_len, "mats"), ctypes.c_void_p(vecs64_cols.data_ptr()),
            ctypes.c_void_p(sol_cols.data_ptr()), num_rhs, int(iterations), 1 if from_zero else 0,
            self._ptr(gains, self.batch, s.gains_len, "gains"), ctypes.c_void_p(self.workspace.data_ptr()),
            ctypes.c_void_p(self._col_ws.data_ptr()), ctypes.c_void_p(self._refine_multi_ws.data_ptr()),
            ctypes.c_void_p(self.status.data_ptr() if use_status else None), ctypes.c_void_p(norms.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_refine_multi")
        return sol_cols, norms

    def vjp_mats(self, sol, adj, use_status=True, grad_mats=None, stream=None):
        """dL/dmats [batch, mats_len] in the plan's layout from the solution and the adjoint (sip_lqr_vjp_mats): sol and
        adj both in the plan's dtype or both float64, and the gradient in that dtype.  Problems whose factor status is
        not SUCCESS get zeros (use_status=False: nothing is masked)."""
        s = self.shape
        wide = self._wide(sol, adj)
        if grad_mats is None:
            grad_mats = torch.empty(self.batch, s.mats_len, dtype=sol.dtype, device=self.device)
        elif grad_mats.dtype != sol.dtype or grad_mats.device != self.device or not grad_mats.is_contiguous() \
                or grad_mats.numel() != self.batch * s.mats_len:
            raise ValueError(f"grad_mats: expected contiguous {sol.dtype} [{self.batch}, {s.mats_len}] on {self.device}")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_vjp_mats(
            self._plan, ctypes.c_void_p(sol.data_ptr()), ctypes.c_void_p(adj.data_ptr()), wide,
            ctypes.c_void_p(self.status.data_ptr() if use_status else None), ctypes.c_void_p(grad_mats.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_vjp_mats")
        return grad_mats

    def vjp(self, mats, sol, grad_sol, gains, want_mats=True, use_status=True, refine_iterations=0, stream=None):
        """The backward pass of the solve against the last factor(): (grad_mats or None, grad_vecs) of a loss whose
        gradient with respect to `sol` is grad_sol.  grad_vecs is the adjoint lambda (K lambda + grad_sol = 0), grad_mats
        the outer products of include/sip_lqr_amd.h in the plan's layout; the gains are not differentiated.
        refine_iterations = 0: one sip_lqr_vjp call, everything in the plan's dtype.  refine_iterations > 0: lambda
        from refine() on the float64 grad_sol, the kernel on float64 sol and lambda, float64 gradients (the accurate
        path of fp32 plans).  Problems whose factor status is not SUCCESS get zeros (use_status=False: whatever their
        solve leaves)."""
        s = self.shape
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        if refine_iterations > 0:
            grad_vecs, _ = self.refine(mats, grad_sol.double().contiguous(), gains, iterations=refine_iterations,
                                       use_status=use_status, stream=stream)
            grad_mats = self.vjp_mats(sol.double().contiguous(), grad_vecs, use_status=use_status, stream=stream) \
                if want_mats else None
            return grad_mats, grad_vecs
        grad_vecs = self.empty_sol()
        grad_mats = torch.empty(self.batch, s.mats_len, dtype=self.dtype, device=self.device) if want_mats else None
        _check(self._lib.sip_lqr_vjp(
            self._plan, self._ptr(mats, self.batch, s.mats_len, "mats"), self._ptr(sol, self.batch, s.vecs_len, "sol"),
            self._ptr(grad_sol, self.batch, s.vecs_len, "grad_sol"), self._ptr(gains, self.batch, s.gains_len, "gains"),
            ctypes.c_void_p(self.workspace.data_ptr()), ctypes.c_void_p(self.status.data_ptr() if use_status else None),
            ctypes.c_void_p(grad_vecs.data_ptr()), ctypes.c_void_p(grad_mats.data_ptr() if want_mats else None),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_vjp")
        return grad_mats, grad_vecs

    @property
    def vjp_multi_columns(self):
        """Columns one launch of vjp_mats_multi carries on this plan (sip_lqr_vjp_multi_columns)."""
        return int(self._lib.sip_lqr_vjp_multi_columns(self._plan))

    def _grad_mats(self, grad_mats, dtype):
        s = self.shape
        if grad_mats is None:
            return torch.empty(self.batch, s.mats_len, dtype=dtype, device=self.device)
        if grad_mats.dtype != dtype or grad_mats.device != self.device or not grad_mats.is_contiguous() \
                or grad_mats.numel() != self.batch * s.mats_len:
            raise ValueError(f"grad_mats: expected contiguous {dtype} [{self.batch}, {s.mats_len}] on {self.device}")
        return grad_mats

    def vjp_mats_multi(self, sol_cols, adj_cols, use_status=True, grad_mats=None, stream=None):
        """dL/dmats [batch, mats_len] of a loss that reads several solutions against one `mats`: the sum over the
        columns of vjp_mats, formed in the kernel (sip_lqr_vjp_mats_multi).  sol_cols / adj_cols are [num_rhs, batch,
        vecs_len], both in the plan's dtype or both float64, and the gradient in that dtype.  One column gives the
        bits of vjp_mats; no column gives zeros.  Problems whose factor status is not SUCCESS get zeros
        (use_status=False: nothing is masked)."""
        num_rhs = self._cols(sol_cols, "sol_cols", (self.dtype, torch.float64))
        if self._cols(adj_cols, "adj_cols", (sol_cols.dtype,)) != num_rhs:
            raise ValueError("adj_cols: as many columns as sol_cols")
        wide = 1 if sol_cols.dtype == torch.float64 else 0
        grad_mats = self._grad_mats(grad_mats, sol_cols.dtype)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        _check(self._lib.sip_lqr_vjp_mats_multi(
            self._plan, ctypes.c_void_p(sol_cols.data_ptr() if num_rhs else None),
            ctypes.c_void_p(adj_cols.data_ptr() if num_rhs else None), num_rhs, wide,
            ctypes.c_void_p(self.status.data_ptr() if use_status else None), ctypes.c_void_p(grad_mats.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_vjp_mats_multi")
        return grad_mats

    def vjp_multi(self, mats, sol_cols, grad_sol_cols, gains, want_mats=True, use_status=True, refine_iterations=0,
                  stream=None):
        """The backward pass of solve_multi against the last factor(): (grad_mats or None, grad_vecs_cols) of a loss
        whose gradient with respect to sol_cols [num_rhs, batch, vecs_len] is grad_sol_cols.  grad_vecs_cols holds the
        adjoints lambda_c (K lambda_c + grad_sol_c = 0, one solve_multi), grad_mats [batch, mats_len] the sum over the
        columns of vjp's outer products, formed in one kernel.  refine_iterations = 0: one sip_lqr_vjp_multi call,
        everything in the plan's dtype.  refine_iterations > 0: the lambda_c from refine_multi() on the float64
        grad_sol_cols, the kernel on float64 columns, float64 gradients.  Problems whose factor status is not SUCCESS
        get zeros (use_status=False: whatever their solve leaves)."""
        s = self.shape
        num_rhs = self._cols(sol_cols, "sol_cols", (self.dtype,))
        if self._cols(grad_sol_cols, "grad_sol_cols", (self.dtype,)) != num_rhs:
            raise ValueError("grad_sol_cols: as many columns as sol_cols")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        if refine_iterations > 0:
            grad_vecs_cols, _ = self.refine_multi(mats, grad_sol_cols.double().contiguous(), gains,
                                                  iterations=refine_iterations, use_status=use_status, stream=stream)
            grad_mats = self.vjp_mats_multi(sol_cols.double().contiguous(), grad_vecs_cols, use_status=use_status,
                                            stream=stream) if want_mats else None
            return grad_mats, grad_vecs_cols
        grad_vecs_cols = torch.empty(num_rhs, self.batch, s.vecs_len, dtype=self.dtype, device=self.device)
        grad_mats = self._grad_mats(None, self.dtype) if want_mats else None
        need = self._lib.sip_lqr_solve_multi_workspace_bytes(self._plan, num_rhs)
        if getattr(self, "_col_ws", None) is None or self._col_ws.numel() < need:
            self._col_ws = torch.empty(max(1, need), dtype=torch.uint8, device=self.device)
        _check(self._lib.sip_lqr_vjp_multi(
            self._plan, self._ptr(mats, self.batch, s.mats_len, "mats"),
            ctypes.c_void_p(sol_cols.data_ptr() if num_rhs else None),
            ctypes.c_void_p(grad_sol_cols.data_ptr() if num_rhs else None), num_rhs,
            self._ptr(gains, self.batch, s.gains_len, "gains"), ctypes.c_void_p(self.workspace.data_ptr()),
            ctypes.c_void_p(self._col_ws.data_ptr()), ctypes.c_void_p(self.status.data_ptr() if use_status else None),
            ctypes.c_void_p(grad_vecs_cols.data_ptr() if num_rhs else self._col_ws.data_ptr()),
            ctypes.c_void_p(grad_mats.data_ptr() if want_mats else None),
            ctypes.c_void_p(stream.cuda_stream)), "sip_lqr_vjp_multi")
        return grad_mats, grad_vecs_cols

    def close(self):
        if getattr(self, "_plan", None):
            self._lib.sip_lqr_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
