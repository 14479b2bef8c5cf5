!
! examples/fortran_sparse_gen_caller/sparse_gen_caller.f90 -- a Fortran caller with a SPARSE PENCIL A x = lambda B x (stiffness
! and mass matrix, Hamiltonian and overlap matrix) that lives on the device.
!
! examples/fortran_sparse_caller carried on to the generalised drivers: the caller assembles A and B once in CSR form on the host,
! hands A to the library's sparse operator (include/diaglib_amd.h: dla_spmm_setup_csr) and B to the metric slot beside it
! (dla_spmm_setup_metric_csr), switches the drivers to device callbacks and passes the three entry points -- bind(C) routines with
! the reference's matvec(n,m,x,ax) / precnd(n,m,fac,x,px) / bvec(n,m,x,bx) shapes that take DEVICE addresses -- where the host
! routines of examples/fortran_gen_caller go.  gen_david_driver (reference diaglib.f90:1855) and lobpcg_driver with
! gen_eig = .true. (:171) are called through the unmodified module interface; panels, both matrices and the preconditioner stay
! in HBM.  The preconditioner is the harness' x / (a_ii + fac), which the reference harness passes for the generalised problem
! too (main.f90:491-492); dla_spmm_precnd_pencil, x / (a_ii + fac b_ii), has the same shape and could stand in its place.
!
! A is the reference's test matrix made sparse (main.f90:311-317): a_ii = i + 1, a_ij = 1/(i+j) for |i-j| <= 6.
! B: b_ii = 1 + 0.25 sin^2(0.003 (i-1)), b_ij = 0.15/k cos(0.01 (min(i,j)-1)) for k = |i-j| = 1, 2 -- strictly diagonally
! dominant (off-diagonal row sums below 0.45), hence positive definite.
!
program sparse_gen_caller
  use real_precision
  use iso_c_binding
  use diaglib, only : gen_david_driver, lobpcg_driver, diaglib_amd_config
  implicit none
  interface
    function dla_default_ctx() bind(C,name='dla_default_ctx') result(ctx)
      import :: c_ptr
      type(c_ptr) :: ctx
    end function
    function dla_spmm_setup_csr(ctx,n,rowptr,colind,values) bind(C,name='dla_spmm_setup_csr') result(st)
      import :: c_ptr, c_int, c_long_long, c_double
      type(c_ptr), value   :: ctx
      integer(c_int), value :: n
      integer(c_long_long) :: rowptr(*)
      integer(c_int)       :: colind(*)
      real(c_double)       :: values(*)
      integer(c_int)       :: st
    end function
    function dla_spmm_setup_metric_csr(ctx,n,rowptr,colind,values,fmt) bind(C,name='dla_spmm_setup_metric_csr') result(st)
      import :: c_ptr, c_int, c_long_long, c_double
      type(c_ptr), value   :: ctx
      integer(c_int), value :: n, fmt
      integer(c_long_long) :: rowptr(*)
      integer(c_int)       :: colind(*)
      real(c_double)       :: values(*)
      integer(c_int)       :: st
    end function
    subroutine dla_spmm_matvec(n,m,x,ax) bind(C,name='dla_spmm_matvec')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), ax(*)
    end subroutine
    subroutine dla_spmm_bvec(n,m,x,bx) bind(C,name='dla_spmm_bvec')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), bx(*)
    end subroutine
    subroutine dla_spmm_precnd(n,m,fac,x,px) bind(C,name='dla_spmm_precnd')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: fac, x(*), px(*)
    end subroutine
    subroutine dla_last_solve_info(iters,matvec_cols,restarts) bind(C,name='dla_last_solve_info')
      import :: c_int
      integer(c_int) :: iters, matvec_cols, restarts
    end subroutine
  end interface
  integer, parameter  :: n = 4000, half = 6, n_want = 6, itmax = 300, m_max = 20
  integer(c_int), parameter :: fmt_ell = 0          ! DLA_SPMM_ELL (1 = sliced ELLPACK, 2 = the library chooses)
  real(dp), parameter :: tol = 1.0e-9_dp
  integer  :: n_eig, i, j, k, nnz
  logical  :: ok
  integer(c_long_long), allocatable :: ia(:), ib(:)
  integer(c_int),       allocatable :: ja(:), jb(:)
  real(dp),             allocatable :: va(:), vb(:), eig(:), evec(:,:), guess(:,:), ax(:), bx(:)
!
! CSR assembly of both matrices, 0-based indices as the C interface wants them
!
  allocate (ia(n+1), ja(n*(2*half+1)), va(n*(2*half+1)), ib(n+1), jb(5*n), vb(5*n))
  nnz = 0
  ia(1) = 0
  do i = 1, n
    do j = max(1,i-half), min(n,i+half)
      nnz = nnz + 1
      ja(nnz) = j - 1
      if (j.eq.i) then
        va(nnz) = real(i+1,dp)
      else
        va(nnz) = 1.0_dp/real(i+j,dp)
      end if
    end do
    ia(i+1) = nnz
  end do
  nnz = 0
  ib(1) = 0
  do i = 1, n
    do j = max(1,i-2), min(n,i+2)
      nnz = nnz + 1
      jb(nnz) = j - 1
      k = abs(i-j)
      if (k.eq.0) then
        vb(nnz) = 1.0_dp + 0.25_dp*sin(0.003_dp*real(i-1,dp))**2
      else
        vb(nnz) = 0.15_dp/real(k,dp)*cos(0.01_dp*real(min(i,j)-1,dp))
      end if
    end do
    ib(i+1) = nnz
  end do
  if (dla_spmm_setup_csr(dla_default_ctx(), n, ia, ja, va).ne.0) stop 'operator setup failed'
  if (dla_spmm_setup_metric_csr(dla_default_ctx(), n, ib, jb, vb, fmt_ell).ne.0) stop 'metric setup failed'
  call diaglib_amd_config(callbacks_on_device=.true., evec_on_device=.false.)
!
  n_eig = min(2*n_want, n_want+5)
  allocate (eig(n_eig), evec(n,n_eig), guess(n,n_eig), ax(n), bx(n))
  call random_number(guess)
  guess = guess - 0.5_dp
  guess(201:,:) = 1.0e-3_dp*guess(201:,:)
!
! Davidson-Liu with the metric (caller of the reference: main.f90:403-526)
!
  evec = guess
  call gen_david_driver(.false.,n,n_want,n_eig,itmax,tol,m_max,0.0_dp,dla_spmm_matvec,dla_spmm_precnd,dla_spmm_bvec,eig,evec,ok)
  call report('SPARSE GEN_DAVIDSON')
!
! the same problem with LOBPCG
!
  evec = guess
  call lobpcg_driver(.false.,.true.,n,n_want,n_eig,itmax,tol,0.0_dp,dla_spmm_matvec,dla_spmm_precnd,dla_spmm_bvec,eig,evec,ok)
  call report('SPARSE GEN_LOBPCG')
  call diaglib_amd_config(release_cache=.true.)
!
contains
!
! the caller's own check, from the CSR arrays on the host: || A x - eig B x || and x^T B x
!
  subroutine report(tag)
    character(len=*), intent(in) :: tag
    integer(c_int) :: iters, cols, restarts
    real(dp)       :: resmax, orth
    integer        :: r, c
    call dla_last_solve_info(iters, cols, restarts)
    resmax = 0.0_dp
    orth = 0.0_dp
    do c = 1, n_want
      do r = 1, n
        ax(r) = sum(va(ia(r)+1:ia(r+1))*evec(ja(ia(r)+1:ia(r+1))+1,c))
        bx(r) = sum(vb(ib(r)+1:ib(r+1))*evec(jb(ib(r)+1:ib(r+1))+1,c))
      end do
      resmax = max(resmax, sqrt(sum((ax - eig(c)*bx)**2)))
      orth = max(orth, abs(dot_product(evec(:,c), bx) - 1.0_dp))
    end do
    write(6,'(a,a,l2,i6)') tag, ' ok/iterations:', ok, iters
    write(6,'(a,a,6es24.15)') tag, ' eig:', eig(1:n_want)
    write(6,'(a,a,2es12.4)') tag, ' max residual, max |x^T B x - 1|:', resmax, orth
  end subroutine report
end program sparse_gen_caller
