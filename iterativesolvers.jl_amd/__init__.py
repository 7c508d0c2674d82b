"""MI355X-native Krylov inner loop behind IterativeSolvers.jl's cg! / gmres! path.

The directory name (``iterativesolvers.jl_amd``) is not a Python identifier; load it with
``__graft_entry__.load_package()`` (registers it as ``iterativesolvers_jl_amd``).

  csrc/      hand-written HIP kernels (gfx950) + the C ABI of include/mik.h  -> libmik.so
  _lib.py    ctypes binding of that ABI (fails loudly when the library is missing)
  api.py     host-side mirror of the reference interface (cg, cg_, gmres, gmres_, iterables ...): SURVEY section 8 rows only;
             a HipMatrix is an operator too (mul!(y, A::Matrix, x) and adjoint(A): csrc/mik_dense_mul.hip)
  stationary.py  jacobi / gauss_seidel / sor / ssor and their iterables on a HipCSR (src/stationary_sparse.jl)
  stationary_dense.py  the same four on a dense HipMatrix (src/stationary.jl), and the public names that dispatch between the two
  dense_factor.py  what dense_lu.py and dense_chol.py share: the refusals, the handle, ldiv_ / solve, "factor a copy"
  dense_lu.py  lu / lu_ of a dense HipMatrix (partial pivoting on the device) and its ldiv_: the exact Pl / Pr of the reference's tests
  dense_chol.py  cholesky / cholesky_ of a dense HipMatrix, real or complex (lower form, on the device) and its ldiv_: the Pl of test/cg.jl:44-47
  dense_qr.py  qr / qr_ of an m x n dense HipMatrix, m >= n (Householder, on the device): lmul with Q and Q', the least-squares solve, the thin Q, and ldiv (A \\ b)
  svdl.py    svdl: Golub-Kahan-Lanczos SVD with thick restart (src/svdl.jl) on a HipCSR uploaded with its adjoint, or on a HipMatrix
  lobpcg.py  lobpcg: block eigensolver (src/lobpcg.jl) on HipCSR operators, with dense=True also on dense HipMatrix ones, every sweep on a block of columns
  extras.py  solvers outside the scope contract (IDR(s), LSQR, LSMR, QMR, power method); kept apart, unjudged
  dist.py    row-partitioned multi-GPU CG / GMRES (one process per GPU; RCCL, peer-mapped mailboxes, in-process group)
  bench_dist.py  measurement harness of bench.py --gpus N (self-test orchestration, group fall-back, the line) -- not product code
  selftest.py    transport self-test child process
  fixtures.py  the reference's test/benchmark inputs as SparseMatrixCSC arrays
  julia/     the Julia-side shim (ccall bindings + dispatch methods), see INTEGRATION.md
"""
from . import _lib, fixtures                                    # noqa: F401
from ._lib import MikError, lib                                  # noqa: F401
from .api import (CGIterable, CGStateVariables, ClassicalGramSchmidt, ConvergenceHistory, DGKS,   # noqa: F401
                  GenericCGIterable, GenericGMRESIterable, DeviceKrylovOps, GMRESIterable, HipContext, HipCSR, HipMatrix, HipMatrixAdjoint, HipVector, Identity,
                  JacobiPrec, ModifiedGramSchmidt, PCGIterable, cg, cg_, cg_iterator_, default_context,
                  dot, gemv_n_, gmres, gmres_, gmres_iterable_, hessenberg_ldiv_, mul_, niters, norm, nprods,
                  nrests, orthogonalize_and_normalize_, zerox, BiCGStabIterable, bicgstabl, bicgstabl_, bicgstabl_iterator_,
                  gemv_t_, lu_solve_, ChebyshevIterable, chebyshev, chebyshev_, chebyshev_iterable_, MINRESIterable, minres, minres_,
                  minres_iterable_, givens_algorithm, axpy_dot_, axpy2_nrm2_, gram_, LinearOperator, cheb_direction_, minres_update_,
                  bicgstab_mr_update_)
from .stationary import (GaussSeidelIterable, JacobiIterable, PosDefException, SingularException, SORIterable, SSORIterable,   # noqa: F401
                         StationaryOperator)
from .stationary_dense import (DenseGaussSeidelIterable, DenseJacobiIterable, DenseSORIterable, DenseSSORIterable,   # noqa: F401
                               DenseStationaryOperator, gauss_seidel, gauss_seidel_, gauss_seidel_iterable, jacobi, jacobi_,
                               jacobi_iterable, sor, sor_, sor_iterable, ssor, ssor_, ssor_iterable)   # dispatch: HipCSR -> stationary.py
from .dense_lu import DenseLU, lu, lu_                   # noqa: F401
from .dense_chol import DenseCholesky, cholesky, cholesky_   # noqa: F401
from .dense_qr import DenseQR, ldiv, qr, qr_                # noqa: F401
from .svdl import (BrokenArrowBidiagonal, PartialFactorization, svdl, svdl_method_, isconverged, build, thickrestart_,   # noqa: F401
                   harmonicrestart_, extend_, ArgumentError, BoundsError, SvdlBreakdown, SVD)
from .lobpcg import (LOBPCGIterator, LOBPCGResults, LOBPCGState, LobpcgCholeskyError, LobpcgRefusal, lobpcg, lobpcg_)   # noqa: F401
from . import extras                                      # noqa: F401  (beyond SURVEY section 8: IDR(s), LSQR, LSMR, QMR, powm -- unjudged, not re-exported)
