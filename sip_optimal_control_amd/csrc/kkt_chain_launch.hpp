// kkt_chain_launch.hpp -- the table of the Newton-KKT chain kernels (kkt_chain_kernels.hpp,
// kkt_theta_chain_kernels.hpp) for the Newton-KKT C ABI (sip_kkt_amd.hip): one row per instantiation, the generic
// one and one per shape of the reference's benchmark family.  The rows are defined in kkt_chain_kernels.hip; a unit
// that only looks a row up and launches through it instantiates no chain kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kkt_chain_kernels.hpp"
#include "kkt_kernels.hpp"
#include "kkt_theta_kernels.hpp"
#include "kkt_theta_chain_kernels.hpp"

// The benchmark family (kkt_chain_kernels.hpp: family_dims), stated here and nowhere else: its state dimensions,
// and the shapes (N, M) of one of them.  kkt_chain_kernels.hip compiles once per state dimension.
#define SIP_KKT_FAMILY_N(X) X(4) X(6) X(8) X(12)
#define SIP_KKT_FAMILY_SHAPES(X, N) X(N, 1) X(N, 2) X(N, 3) X(N, 4)

namespace sipamd {
namespace kkt {

// the signature every instantiation of a kernel template shares, parameters as at the kernel's definition (the
// templates' default arguments do not travel with a pointer: a launch through a row passes every argument)
typedef void (*condense_chain_t)(ChainKkt, const double *, const double *, const double *, double *, const double *,
                                 double *, long, const int32_t *, int, long, long);
typedef void (*condense_chain_pipe_t)(ChainKkt, const double *, const double *, const double *, double *,
                                      const double *, double *, long, int);
typedef void (*recover_chain_t)(ChainKkt, const double *, const double *, const double *, const double *, double *,
                                const int32_t *, long, int, long, long, long);
typedef void (*apply_chain_t)(ChainKkt, int, const double *, const double *, const double *, const double *,
                              const double *, ApplyIO, long);
typedef void (*apply_theta_chain_t)(ChainKkt, ChainTheta, const double *, const double *, ApplyIO, long);
typedef void (*theta_rhs_chain_t)(ChainKkt, ChainTheta, const double *, const double *, const double *, double *, long,
                                  const int32_t *, long);
typedef void (*theta_recover_chain_t)(ChainKkt, ChainTheta, const double *, const double *, const double *,
                                      const double *, long, double *, long, double *, const int32_t *, long);
typedef void (*theta_dot_chain_t)(ChainKkt, ChainTheta, const double *, const double *, double *, const int32_t *, long);

struct KktChainKernels {
  int n, m; // the family shape the kernels of the row hold as constants; (0, 0): the generic instantiation
  condense_chain_t condense_rhs, condense, rhs; // <WITH_RHS, MATS> = <true, true>, <false, true>, <true, false>
  condense_chain_pipe_t condense_pipe_rhs, condense_pipe; // <WITH_RHS> = <true>, <false>
  recover_chain_t recover, recover_cols;                  // <COLS> = <false>, <true>
  apply_chain_t apply;
  apply_theta_chain_t apply_theta;
  theta_rhs_chain_t theta_rhs;
  theta_recover_chain_t theta_recover;
  theta_dot_chain_t theta_dot;
};

// The row of the instantiation <N, M>: defined, and its kernels with it, in kkt_chain_kernels.hip alone.
template <int N, int M>
extern const KktChainKernels kkt_chain_row;
#define SIP_KKT_DECLARE_ROW(N, M) extern template const KktChainKernels kkt_chain_row<N, M>;
#define SIP_KKT_DECLARE_ROWS(N) SIP_KKT_FAMILY_SHAPES(SIP_KKT_DECLARE_ROW, N)
SIP_KKT_DECLARE_ROW(0, 0) SIP_KKT_FAMILY_N(SIP_KKT_DECLARE_ROWS)
#undef SIP_KKT_DECLARE_ROWS
#undef SIP_KKT_DECLARE_ROW

// The row of the family shape (n, m); the generic row where the family has no such shape (sip_kkt_amd.hip).
const KktChainKernels *find_kkt_chain_kernels(int n, int m);

} // namespace kkt
} // namespace sipamd
