"""The solves as differentiable torch functions: sol = chain_lqr_solve(solver, mats, vecs), sol_cols =
chain_lqr_solve_multi(solver, mats, vecs_cols), output = tree_lqr_solve(solver, input) and out_cols =
tree_lqr_solve_multi(solver, input, rhs_cols).  The chain first; the tree twins follow the same scheme (below).

Forward is solver.factor(mats) + solver.solve(...); backward is one adjoint solve against that factorisation and the
outer-product kernel (BatchedChainLQR.vjp, sip_lqr_vjp), all on the device.  The factor state lives in the solver's
workspace, which later factor* calls overwrite: forward remembers the solver's factor_generation, and a backward pass
that finds another value factors the saved mats again before it solves -- stale state is never used.  The gains are
not differentiated, and there is no second derivative (backward is once_differentiable)."""
import torch
from torch.autograd.function import once_differentiable


class _ChainLQRSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, mats, vecs):
        gains, status = solver.factor(mats)
        sol = solver.solve(mats, vecs, gains)
        ctx.solver = solver
        ctx.generation = solver.factor_generation
        ctx.save_for_backward(mats, sol, gains)
        status = status.clone()  # the solver's own buffer is rewritten by the next factor call
        ctx.mark_non_differentiable(status)
        return sol, status

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_sol, _grad_status):
        solver = ctx.solver
        mats, sol, gains = ctx.saved_tensors
        if solver.factor_generation != ctx.generation:  # someone factored since: the workspace is not ours any more
            solver.factor(mats, gains)
            ctx.generation = solver.factor_generation
        want_mats = ctx.needs_input_grad[1]
        grad_mats, grad_vecs = solver.vjp(mats, sol, grad_sol.contiguous(), gains, want_mats=want_mats)
        return None, grad_mats, grad_vecs if ctx.needs_input_grad[2] else None


def chain_lqr_solve(solver, mats, vecs, return_status=False):
    """sol [batch, vecs_len] of `solver` (a BatchedChainLQR) on mats, vecs, differentiable with respect to both.
    return_status=True: (sol, status), status the int32 factor statuses of this call (not differentiable); a problem
    whose status is not SUCCESS has an unspecified sol and gets zero gradients."""
    sol, status = _ChainLQRSolve.apply(solver, mats, vecs)
    return (sol, status) if return_status else sol


class _ChainLQRSolveMulti(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, mats, vecs_cols):
        gains, status = solver.factor(mats)
        sol_cols = solver.solve_multi(mats, vecs_cols, gains)
        ctx.solver = solver
        ctx.generation = solver.factor_generation
        ctx.save_for_backward(mats, sol_cols, gains)
        status = status.clone()  # the solver's own buffer is rewritten by the next factor call
        ctx.mark_non_differentiable(status)
        return sol_cols, status

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_sol_cols, _grad_status):
        solver = ctx.solver
        mats, sol_cols, gains = ctx.saved_tensors
        if solver.factor_generation != ctx.generation:  # someone factored since: the workspace is not ours any more
            solver.factor(mats, gains)
            ctx.generation = solver.factor_generation
        want_mats = ctx.needs_input_grad[1]
        grad_mats, grad_vecs_cols = solver.vjp_multi(mats, sol_cols, grad_sol_cols.contiguous(), gains,
                                                     want_mats=want_mats)
        return None, grad_mats, grad_vecs_cols if ctx.needs_input_grad[2] else None


def chain_lqr_solve_multi(solver, mats, vecs_cols, return_status=False):
    """sol_cols [num_rhs, batch, vecs_len] of `solver` (a BatchedChainLQR) on one mats and the right-hand sides
    vecs_cols [num_rhs, batch, vecs_len], differentiable with respect to both.  Forward is solver.factor(mats) +
    solver.solve_multi(...); backward is one solver.vjp_multi (sip_lqr_vjp_multi): one adjoint solve_multi, and the
    gradient of mats summed over the columns in one kernel.  The factor_generation check is that of chain_lqr_solve.
    return_status=True: (sol_cols, status), status the int32 factor statuses of this call (not differentiable); a
    problem whose status is not SUCCESS has unspecified columns and gets zero gradients."""
    sol_cols, status = _ChainLQRSolveMulti.apply(solver, mats, vecs_cols)
    return (sol_cols, status) if return_status else sol_cols


class _TreeLQRSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, input):
        solver.input.copy_(input.detach().reshape(solver.input.shape))
        solver.factor_fused()
        solver.solve_fused()
        ctx.solver = solver
        ctx.generation = solver.factor_generation
        output, status = solver.output.clone(), solver.status.clone()  # the solver's own buffers are rewritten later
        ctx.save_for_backward(input.detach().clone(), output)
        ctx.mark_non_differentiable(status)
        return output, status

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output, _grad_status):
        solver = ctx.solver
        input, output = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None
        if solver.factor_generation != ctx.generation:  # someone packed or factored since: neither arena is ours
            solver.input.copy_(input.reshape(solver.input.shape))
            solver.factor_fused()
            ctx.generation = solver.factor_generation
        grad_input, _ = solver.vjp(grad_output.contiguous(), output=output, want_input=True)
        return None, grad_input.reshape(input.shape)


def tree_lqr_solve(solver, input, return_status=False):
    """output [batch, output_len] of `solver` (a BatchedTreeLQR) on `input` [batch, in_len] (the input arena: node
    blocks Q | q | c | delta, edge blocks A | B | M | R | r, as pack() writes them), differentiable with respect to it.
    Forward copies `input` into solver.input and runs factor_fused() + solve_fused(); backward is one solver.vjp
    (sip_lqr_tree_vjp).  Forward remembers solver.factor_generation, which pack() and every factor* call bump: a
    backward pass that finds another value copies the saved input back and factors again first, so stale factor state
    or a foreign input arena is never used.  return_status=True: (output, status), status the int32 factor statuses of
    this call (not differentiable); a problem whose status is not SUCCESS has an unspecified output and gets zero
    gradients.  The gains are not differentiated, and there is no second derivative."""
    output, status = _TreeLQRSolve.apply(solver, input)
    return (output, status) if return_status else output


class _TreeLQRSolveMulti(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, input, rhs_cols):
        solver.input.copy_(input.detach().reshape(solver.input.shape))
        solver.factor_fused()
        out_cols = solver.solve_multi(rhs_cols.detach())
        ctx.solver = solver
        ctx.generation = solver.factor_generation
        status = solver.status.clone()  # the solver's own buffer is rewritten by the next factor call
        ctx.save_for_backward(input.detach().clone(), out_cols)
        ctx.mark_non_differentiable(status)
        return out_cols, status

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out_cols, _grad_status):
        solver = ctx.solver
        input, out_cols = ctx.saved_tensors
        want_input, want_rhs = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (want_input or want_rhs):
            return None, None, None
        if solver.factor_generation != ctx.generation:  # someone packed or factored since: neither arena is ours
            solver.input.copy_(input.reshape(solver.input.shape))
            solver.factor_fused()
            ctx.generation = solver.factor_generation
        grad_input, adj_cols = solver.vjp_multi(grad_out_cols.contiguous(), out_cols, want_input=want_input)
        return None, grad_input.reshape(input.shape) if want_input else None, adj_cols if want_rhs else None


def tree_lqr_solve_multi(solver, input, rhs_cols, return_status=False):
    """out_cols [num_rhs, batch, output_len] of `solver` (a BatchedTreeLQR) on one `input` [batch, in_len] (the input
    arena) and the right-hand sides rhs_cols [num_rhs, batch, rhs_len] (pack_rhs), differentiable with respect to both.
    Forward copies `input` into solver.input and runs factor_fused() + solve_multi(rhs_cols); backward is one
    solver.vjp_multi (sip_lqr_tree_vjp_multi): one adjoint solve_multi, and the gradient of the input arena summed over
    the columns in one kernel.  solve_multi does not read the arena's q, c, r, so their slots of the gradient are zero;
    the gradient of rhs_cols is the adjoint columns.  The factor_generation check is that of tree_lqr_solve.
    return_status=True: (out_cols, status), status the int32 factor statuses of this call (not differentiable); a
    problem whose status is not SUCCESS has unspecified columns and gets zero gradients."""
    out_cols, status = _TreeLQRSolveMulti.apply(solver, input, rhs_cols)
    return (out_cols, status) if return_status else out_cols
