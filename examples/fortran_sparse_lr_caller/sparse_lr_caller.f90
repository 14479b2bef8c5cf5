!
! examples/fortran_sparse_lr_caller/sparse_lr_caller.f90 -- a Fortran caller with a SPARSE LINEAR-RESPONSE PENCIL
!   (A B; B A)(Y Z) = w (S D; -D -S)(Y Z)
! that lives on the device.
!
! examples/fortran_sparse_gen_caller carried on to the linear-response drivers: the caller assembles A+B, A-B, S+D and S-D once
! in CSR form on the host, hands them to the four part slots of the library (include/diaglib_amd.h: dla_spmm_setup_lr_csr with
! part 0 .. 3), switches the drivers to device callbacks and passes the library's entry points -- bind(C) routines with the
! reference's apbmul / ambmul / spdmul / smdmul (n,m,x,y) and lrprec (n,m,fac,xp,xm,yp,ym) shapes that take DEVICE addresses --
! where the host routines of examples/fortran_caller go.  caslr_eff_driver (reference diaglib.f90:1024) and caslr_driver (:558)
! are called through the unmodified module interface; panels, the four matrices and the preconditioner stay in HBM.  The
! preconditioners are the harness' lrprec_2 for caslr_eff_driver and lrprec_1 for caslr_driver (main.f90:234-281) on the diagonals
! of the stored matrices.
!
! The matrices (1-based i, j; k = |i-j|):
!   E_ij  = 0.05 sin(i+j)           for k = 1, 2, 3          (symmetric)
!   A+B   = diag(i + 5) + E,   A-B = diag(i + 2) + 0.2 E
!   S     = diag(1 + 0.5/(1 + mod(i,7))) + 0.0005 cos(i+j)  for k = 1, 2
!   D_ij  = 0.02 sin(0.3 (i+j)) sign(j-i)  for k = 1, 2      (antisymmetric)
! A+B, A-B and S are strictly diagonally dominant, hence positive definite.
!
program sparse_lr_caller
  use real_precision
  use iso_c_binding
  use diaglib, only : caslr_eff_driver, caslr_driver, diaglib_amd_config
  implicit none
  interface
    function dla_default_ctx() bind(C,name='dla_default_ctx') result(ctx)
      import :: c_ptr
      type(c_ptr) :: ctx
    end function
    function dla_spmm_setup_lr_csr(ctx,part,n,rowptr,colind,values,fmt) bind(C,name='dla_spmm_setup_lr_csr') result(st)
      import :: c_ptr, c_int, c_long_long, c_double
      type(c_ptr), value   :: ctx
      integer(c_int), value :: part, n, fmt
      integer(c_long_long) :: rowptr(*)
      integer(c_int)       :: colind(*)
      real(c_double)       :: values(*)
      integer(c_int)       :: st
    end function
    function dla_spmm_drop_lr(ctx) bind(C,name='dla_spmm_drop_lr') result(st)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx
      integer(c_int)     :: st
    end function
    subroutine dla_spmm_apbmul(n,m,x,y) bind(C,name='dla_spmm_apbmul')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), y(*)
    end subroutine
    subroutine dla_spmm_ambmul(n,m,x,y) bind(C,name='dla_spmm_ambmul')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), y(*)
    end subroutine
    subroutine dla_spmm_spdmul(n,m,x,y) bind(C,name='dla_spmm_spdmul')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), y(*)
    end subroutine
    subroutine dla_spmm_smdmul(n,m,x,y) bind(C,name='dla_spmm_smdmul')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), y(*)
    end subroutine
    subroutine dla_spmm_lrprec1(n,m,fac,xp,xm,yp,ym) bind(C,name='dla_spmm_lrprec1')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: fac, xp(*), xm(*), yp(*), ym(*)
    end subroutine
    subroutine dla_spmm_lrprec2(n,m,fac,xp,xm,yp,ym) bind(C,name='dla_spmm_lrprec2')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: fac, xp(*), xm(*), yp(*), ym(*)
    end subroutine
    subroutine dla_last_solve_info(iters,matvec_cols,restarts) bind(C,name='dla_last_solve_info')
      import :: c_int
      integer(c_int) :: iters, matvec_cols, restarts
    end subroutine
  end interface
  integer, parameter  :: n = 300, half = 3, n_want = 4, itmax = 100, m_max = 20
  integer(c_int), parameter :: fmt_ell = 0, fmt_sell = 1     ! DLA_SPMM_ELL, DLA_SPMM_SELL (2 = the library chooses)
  integer(c_int), parameter :: p_apb = 0, p_amb = 1, p_spd = 2, p_smd = 3
  real(dp), parameter :: tol = 1.0e-9_dp
  integer  :: n_eig, i, j, k, nnz
  logical  :: ok
  real(dp) :: e, s, d
  integer(c_long_long), allocatable :: ip(:)
  integer(c_int),       allocatable :: jp(:)
  real(dp),             allocatable :: vapb(:), vamb(:), vspd(:), vsmd(:), w(:), xy(:,:), guess(:,:), lhs(:), rhs(:), vp(:), vm(:)
!
! CSR assembly, 0-based indices as the C interface wants them: the four matrices share one pattern here (|i-j| <= 3), which
! the library does not require
!
  allocate (ip(n+1), jp(n*(2*half+1)), vapb(n*(2*half+1)), vamb(n*(2*half+1)), vspd(n*(2*half+1)), vsmd(n*(2*half+1)))
  nnz = 0
  ip(1) = 0
  do i = 1, n
    do j = max(1,i-half), min(n,i+half)
      k = abs(i-j)
      nnz = nnz + 1
      jp(nnz) = j - 1
      if (k.eq.0) then
        vapb(nnz) = real(i+5,dp)
        vamb(nnz) = real(i+2,dp)
        vspd(nnz) = 1.0_dp + 0.5_dp/real(1+mod(i,7),dp)
        vsmd(nnz) = vspd(nnz)
      else
        e = 0.05_dp*sin(real(i+j,dp))
        s = 0.0_dp
        d = 0.0_dp
        if (k.le.2) then
          s = 0.0005_dp*cos(real(i+j,dp))
          d = 0.02_dp*sin(0.3_dp*real(i+j,dp))
          if (j.lt.i) d = -d
        end if
        vapb(nnz) = e
        vamb(nnz) = 0.2_dp*e
        vspd(nnz) = s + d
        vsmd(nnz) = s - d
      end if
    end do
    ip(i+1) = nnz
  end do
  if (dla_spmm_setup_lr_csr(dla_default_ctx(), p_apb, n, ip, jp, vapb, fmt_ell).ne.0) stop 'A+B setup failed'
  if (dla_spmm_setup_lr_csr(dla_default_ctx(), p_amb, n, ip, jp, vamb, fmt_ell).ne.0) stop 'A-B setup failed'
  if (dla_spmm_setup_lr_csr(dla_default_ctx(), p_spd, n, ip, jp, vspd, fmt_sell).ne.0) stop 'S+D setup failed'
  if (dla_spmm_setup_lr_csr(dla_default_ctx(), p_smd, n, ip, jp, vsmd, fmt_sell).ne.0) stop 'S-D setup failed'
  call diaglib_amd_config(callbacks_on_device=.true., evec_on_device=.false.)
!
  n_eig = min(2*n_want, n_want+5)
  allocate (w(n_eig), xy(2*n,n_eig), guess(2*n,n_eig), lhs(2*n), rhs(2*n), vp(n), vm(n))
!
! guess: sin(0.37 i j + j), concentrated on the first 40 rows (unit vectors would leave the first expansions of these narrow
! bands with compact support, and the block rank-deficient)
!
  do j = 1, n_eig
    do i = 1, 2*n
      guess(i,j) = sin(0.37_dp*real(i*j,dp) + real(j,dp))
      if (i.gt.40) guess(i,j) = 1.0e-2_dp*guess(i,j)
    end do
  end do
!
! the efficient driver (caller of the reference: main.f90:528-730) ...
!
  xy = guess
  call caslr_eff_driver(.false.,n,2*n,n_want,n_eig,itmax,tol,m_max,dla_spmm_apbmul,dla_spmm_ambmul,dla_spmm_spdmul, &
                        dla_spmm_smdmul,dla_spmm_lrprec2,w,xy,ok)
  call report('SPARSE CASLR_EFF')
!
! ... and the traditional one on the same matrices
!
  xy = guess
  call caslr_driver(.false.,n,2*n,n_want,n_eig,itmax,tol,m_max,dla_spmm_apbmul,dla_spmm_ambmul,dla_spmm_spdmul, &
                    dla_spmm_smdmul,dla_spmm_lrprec1,w,xy,ok)
  call report('SPARSE CASLR')
  if (dla_spmm_drop_lr(dla_default_ctx()).ne.0) stop 'drop failed'
  call diaglib_amd_config(release_cache=.true.)
!
contains
!
! the caller's own check, from the CSR arrays on the host: with v+ = Y + Z, v- = Y - Z the pencil reads
!   (A+B) v+ = w (S-D) v-   and   (A-B) v- = w (S+D) v+      (reference diaglib.f90:1027-1046)
!
  subroutine report(tag)
    character(len=*), intent(in) :: tag
    integer(c_int) :: iters, cols, restarts
    real(dp)       :: resmax
    integer        :: r, c
    call dla_last_solve_info(iters, cols, restarts)
    resmax = 0.0_dp
    do c = 1, n_want
      vp = xy(1:n,c) + xy(n+1:2*n,c)
      vm = xy(1:n,c) - xy(n+1:2*n,c)
      do r = 1, n
        lhs(r)   = sum(vapb(ip(r)+1:ip(r+1))*vp(jp(ip(r)+1:ip(r+1))+1))
        rhs(r)   = sum(vsmd(ip(r)+1:ip(r+1))*vm(jp(ip(r)+1:ip(r+1))+1))
        lhs(n+r) = sum(vamb(ip(r)+1:ip(r+1))*vm(jp(ip(r)+1:ip(r+1))+1))
        rhs(n+r) = sum(vspd(ip(r)+1:ip(r+1))*vp(jp(ip(r)+1:ip(r+1))+1))
      end do
      resmax = max(resmax, sqrt(sum((lhs - w(c)*rhs)**2))/sqrt(sum(lhs**2)))
    end do
    write(6,'(a,a,l2,i6)') tag, ' ok/iterations:', ok, iters
    write(6,'(a,a,4es24.15)') tag, ' eig:', w(1:n_want)
    write(6,'(a,a,es12.4)') tag, ' max residual:', resmax
  end subroutine report
end program sparse_lr_caller
