!
! examples/fortran_sparse_gen_cheb_caller/sparse_gen_cheb_caller.f90 -- a Fortran caller with a stiffness / mass pair, the
! canonical sparse generalised eigenproblem A x = lambda B x, where a diagonal preconditioner does nothing:
!   A  the five-point -div(kappa grad) on a 32 x 32 grid, row i * 32 + j, kappa(i,j) = 1000 ** (0.5 + 0.5 sin(1.3 i) cos(0.9 j)),
!      harmonic means on the edges and Dirichlet boundaries (the matrix of examples/fortran_sparse_cheb_jacobi_caller);
!   B  a mass matrix on the same pattern: b_ii = rho(i,j) = 1 + 0.5 sin(0.7 i) cos(1.1 j), and every edge carries a tenth of the
!      harmonic mean of its two rho -- off-diagonal row sums of at most 0.8 rho, hence positive definite.
!
! The caller assembles both once in CSR form, hands A to the sparse operator (include/diaglib_amd.h: dla_spmm_setup_csr_fmt) and B
! to the metric beside it (dla_spmm_setup_metric_csr), configures 8 steps with lo_fraction 0.02 (dla_spmm_cheb_config) and passes
! dla_spmm_precnd_cheb_pencil -- the Chebyshev iteration on the scaled pencil D^-1 (A + fac B) -- exactly where a precnd goes, in
! gen_david_driver and in lobpcg_driver with gen_eig = .true., in device mode.  diaglib.f90 is the unmodified module; the interface
! blocks below are this caller's own.  With dla_spmm_precnd_pencil, x / (a_ii + fac b_ii), in its place neither driver reaches the
! tolerance within the 150 iterations allowed here.
!
program sparse_gen_cheb_caller
  use real_precision
  use iso_c_binding
  use diaglib, only : gen_david_driver, lobpcg_driver, diaglib_amd_config
  implicit none
  interface
    function dla_default_ctx() bind(C,name='dla_default_ctx') result(ctx)
      import :: c_ptr
      type(c_ptr) :: ctx
    end function
    function dla_spmm_setup_csr_fmt(ctx,n,rowptr,colind,values,fmt) bind(C,name='dla_spmm_setup_csr_fmt') result(st)
      import :: c_ptr, c_int, c_long_long, c_double
      type(c_ptr), value    :: ctx
      integer(c_int), value :: n, fmt
      integer(c_long_long)  :: rowptr(*)
      integer(c_int)        :: colind(*)
      real(c_double)        :: values(*)
      integer(c_int)        :: st
    end function
    function dla_spmm_setup_metric_csr(ctx,n,rowptr,colind,values,fmt) bind(C,name='dla_spmm_setup_metric_csr') result(st)
      import :: c_ptr, c_int, c_long_long, c_double
      type(c_ptr), value    :: ctx
      integer(c_int), value :: n, fmt
      integer(c_long_long)  :: rowptr(*)
      integer(c_int)        :: colind(*)
      real(c_double)        :: values(*)
      integer(c_int)        :: st
    end function
    function dla_spmm_drop_metric(ctx) bind(C,name='dla_spmm_drop_metric') result(st)
      import :: c_ptr, c_int
      type(c_ptr), value    :: ctx
      integer(c_int)        :: st
    end function
    function dla_spmm_cheb_config(ctx,steps,lo_fraction) bind(C,name='dla_spmm_cheb_config') result(st)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value    :: ctx
      integer(c_int), value :: steps
      real(c_double), value :: lo_fraction
      integer(c_int)        :: st
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
    subroutine dla_spmm_precnd_cheb_pencil(n,m,fac,x,px) bind(C,name='dla_spmm_precnd_cheb_pencil')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: fac, x(*), px(*)
    end subroutine
    subroutine dla_last_solve_info(iters,matvec_cols,restarts) bind(C,name='dla_last_solve_info')
      import :: c_int
      integer(c_int) :: iters, matvec_cols, restarts
    end subroutine
  end interface
  integer, parameter  :: order = 32, n = order*order, n_want = 4, n_eig = 6, itmax = 150, m_max = 10
  integer(c_int), parameter :: fmt_auto = 2         ! DLA_SPMM_AUTO (0 = ELLPACK, 1 = sliced ELLPACK)
  real(dp), parameter :: tol = 1.0e-8_dp, contrast = 1.0e3_dp
  integer  :: i, j, gi, gj, nnz
  logical  :: ok
  integer(c_long_long), allocatable :: rowptr(:)
  integer(c_int),       allocatable :: colind(:)
  real(dp),             allocatable :: va(:), vb(:), eig(:), evec(:,:), guess(:,:), ax(:), bx(:)
!
! CSR assembly of both matrices on one pattern, 0-based indices as the C interface wants them; row gi * order + gj, columns
! ascending.  The diagonal of A is the sum of the row's edge weights, a missing neighbour counting with kappa of the point itself.
!
  allocate (rowptr(n+1), colind(5*n), va(5*n), vb(5*n))
  nnz = 0
  rowptr(1) = 0
  do i = 0, n - 1
    gi = i/order
    gj = mod(i,order)
    if (gi.gt.0)       call entry(i - order, -edge(gi,gj,gi-1,gj), medge(gi,gj,gi-1,gj))
    if (gj.gt.0)       call entry(i - 1, -edge(gi,gj,gi,gj-1), medge(gi,gj,gi,gj-1))
    call entry(i, edge(gi,gj,gi-1,gj) + edge(gi,gj,gi,gj-1) + edge(gi,gj,gi,gj+1) + edge(gi,gj,gi+1,gj), rho(gi,gj))
    if (gj.lt.order-1) call entry(i + 1, -edge(gi,gj,gi,gj+1), medge(gi,gj,gi,gj+1))
    if (gi.lt.order-1) call entry(i + order, -edge(gi,gj,gi+1,gj), medge(gi,gj,gi+1,gj))
    rowptr(i+2) = nnz
  end do
  if (dla_spmm_setup_csr_fmt(dla_default_ctx(), n, rowptr, colind, va, fmt_auto).ne.0) stop 'setup failed'
  if (dla_spmm_setup_metric_csr(dla_default_ctx(), n, rowptr, colind, vb, fmt_auto).ne.0) stop 'metric setup failed'
  if (dla_spmm_cheb_config(dla_default_ctx(), 8, 0.02_dp).ne.0) stop 'configuration failed'
  call diaglib_amd_config(callbacks_on_device=.true., evec_on_device=.false.)
!
! the guess: evec(i,j) = [i = 7 j] + 1e-3 cos(0.7 (i+1)(j+1)), 0-based
!
  allocate (eig(n_eig), evec(n,n_eig), guess(n,n_eig), ax(n), bx(n))
  do j = 0, n_eig - 1
    do i = 0, n - 1
      guess(i+1,j+1) = 1.0e-3_dp*cos(0.7_dp*real(i+1,dp)*real(j+1,dp))
      if (i.eq.7*j) guess(i+1,j+1) = guess(i+1,j+1) + 1.0_dp
    end do
  end do
  evec = guess
  call gen_david_driver(.false.,n,n_want,n_eig,itmax,tol,m_max,0.0_dp,dla_spmm_matvec,dla_spmm_precnd_cheb_pencil,dla_spmm_bvec,eig,evec,ok)
  call report('CHEB-PENCIL GEN_DAVIDSON')
  evec = guess
  call lobpcg_driver(.false.,.true.,n,n_want,n_eig,itmax,tol,0.0_dp,dla_spmm_matvec,dla_spmm_precnd_cheb_pencil,dla_spmm_bvec,eig,evec,ok)
  call report('CHEB-PENCIL GEN_LOBPCG')
  if (dla_spmm_cheb_config(dla_default_ctx(), 0, 0.0_dp).ne.0) stop 'switching the preconditioner off failed'
  if (dla_spmm_drop_metric(dla_default_ctx()).ne.0) stop 'dropping the metric failed'
  call diaglib_amd_config(release_cache=.true.)
!
contains
!
  real(dp) function kappa(a, b)
    integer, intent(in) :: a, b
    kappa = contrast**(0.5_dp + 0.5_dp*sin(1.3_dp*real(a,dp))*cos(0.9_dp*real(b,dp)))
  end function kappa
!
  real(dp) function rho(a, b)
    integer, intent(in) :: a, b
    rho = 1.0_dp + 0.5_dp*sin(0.7_dp*real(a,dp))*cos(1.1_dp*real(b,dp))
  end function rho
!
! the weight of the edge between (a,b) and (c,e): the harmonic mean of kappa, or kappa(a,b) where (c,e) is outside the grid
!
  real(dp) function edge(a, b, c, e)
    integer, intent(in) :: a, b, c, e
    if (c.lt.0 .or. c.ge.order .or. e.lt.0 .or. e.ge.order) then
      edge = kappa(a,b)
    else
      edge = 2.0_dp*kappa(a,b)*kappa(c,e)/(kappa(a,b) + kappa(c,e))
    end if
  end function edge
!
! the mass of the edge between (a,b) and (c,e), both inside the grid: a tenth of the harmonic mean of rho
!
  real(dp) function medge(a, b, c, e)
    integer, intent(in) :: a, b, c, e
    medge = 2.0_dp*rho(a,b)*rho(c,e)/(rho(a,b) + rho(c,e))/10.0_dp
  end function medge
!
  subroutine entry(col, a, b)
    integer,  intent(in) :: col
    real(dp), intent(in) :: a, b
    nnz = nnz + 1
    colind(nnz) = col
    va(nnz) = a
    vb(nnz) = b
  end subroutine entry
!
! the caller's own check, from the CSR arrays on the host: || A x - eig B x ||
!
  subroutine report(tag)
    character(len=*), intent(in) :: tag
    integer(c_int) :: iters, cols, restarts
    integer  :: r, c
    real(dp) :: resmax
    call dla_last_solve_info(iters, cols, restarts)
    resmax = 0.0_dp
    do c = 1, n_want
      do r = 1, n
        ax(r) = sum(va(rowptr(r)+1:rowptr(r+1))*evec(colind(rowptr(r)+1:rowptr(r+1))+1,c))
        bx(r) = sum(vb(rowptr(r)+1:rowptr(r+1))*evec(colind(rowptr(r)+1:rowptr(r+1))+1,c))
      end do
      resmax = max(resmax, sqrt(sum((ax - eig(c)*bx)**2)))
    end do
    write(6,'(a,a,l2,i6)') tag, ' ok/iterations:', ok, iters
    write(6,'(a,a,4es24.15)') tag, ' eig:', eig(1:n_want)
    write(6,'(a,a,es12.4)') tag, ' max residual:', resmax
  end subroutine report
end program sparse_gen_cheb_caller
