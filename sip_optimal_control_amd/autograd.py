"""The chain solve as a differentiable torch function: sol = chain_lqr_solve(solver, mats, vecs).

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
