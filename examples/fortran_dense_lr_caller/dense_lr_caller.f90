!
! examples/fortran_dense_lr_caller/dense_lr_caller.f90 -- a Fortran caller with a DENSE LINEAR-RESPONSE PENCIL
!   (A B; B A)(Y Z) = w (S D; -D -S)(Y Z)
! that lives on the device.
!
! examples/fortran_sparse_lr_caller for a caller that holds dense arrays, the way the reference's own harness does
! (main.f90:528-760).  A CAS-LR or TDDFT-like caller holds A, B, S and D, not their sums and differences: the four arrays are built
! here as such a caller has them and handed over in two calls (include/diaglib_amd.h: dla_dense_setup_lr_pair, pair 0 = A and B,
! pair 1 = S and D), which form A+B, A-B, S+D and S-D while packing the library's own copies -- the arrays could be deallocated
! afterwards.  The drivers are switched to device callbacks and the library's entry points -- bind(C) routines with the reference's
! apbmul / ambmul / spdmul / smdmul (n,m,x,y) and lrprec (n,m,fac,xp,xm,yp,ym) shapes that take DEVICE addresses -- go where the
! host routines of examples/fortran_caller go.  caslr_eff_driver (reference diaglib.f90:1024) and caslr_driver (:558) are called
! through the unmodified module interface; panels, the four matrices and the preconditioner stay in HBM.  The preconditioners are
! the harness' lrprec_2 for caslr_eff_driver and lrprec_1 for caslr_driver (main.f90:234-281) on the stored diagonals.
!
! The matrices (1-based i, j):
!   a_ij = 0.12/(i+j),  a_ii = i + 3.5;    b_ij = 0.08/(i+j),  b_ii = 1.5
!   s_ij = 0.01 cos(i+j)/(1+|i-j|),  s_ii = 1 + 0.5/(1 + mod(i,7))
!   d_ij = 0.02 sin(0.3 (i+j)) sign(j-i)/(1+|i-j|),  d_ii = 0                (antisymmetric)
! A+B, A-B and S are positive definite (smallest eigenvalues 5.99, 3.00 and 1.057).
!
program dense_lr_caller
  use real_precision
  use iso_c_binding
  use diaglib, only : caslr_eff_driver, caslr_driver, diaglib_amd_config
  implicit none
  interface
    function dla_default_ctx() bind(C,name='dla_default_ctx') result(ctx)
      import :: c_ptr
      type(c_ptr) :: ctx
    end function
    function dla_dense_setup_lr_pair(ctx,pair,n,p,ldp,q,ldq) bind(C,name='dla_dense_setup_lr_pair') result(st)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value    :: ctx
      integer(c_int), value :: pair, n, ldp, ldq
      real(c_double)        :: p(ldp,*), q(ldq,*)
      integer(c_int)        :: st
    end function
    function dla_dense_drop_lr(ctx) bind(C,name='dla_dense_drop_lr') result(st)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx
      integer(c_int)     :: st
    end function
    subroutine dla_dense_apbmul(n,m,x,y) bind(C,name='dla_dense_apbmul')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), y(*)
    end subroutine
    subroutine dla_dense_ambmul(n,m,x,y) bind(C,name='dla_dense_ambmul')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), y(*)
    end subroutine
    subroutine dla_dense_spdmul(n,m,x,y) bind(C,name='dla_dense_spdmul')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), y(*)
    end subroutine
    subroutine dla_dense_smdmul(n,m,x,y) bind(C,name='dla_dense_smdmul')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), y(*)
    end subroutine
    subroutine dla_dense_lrprec1(n,m,fac,xp,xm,yp,ym) bind(C,name='dla_dense_lrprec1')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: fac, xp(*), xm(*), yp(*), ym(*)
    end subroutine
    subroutine dla_dense_lrprec2(n,m,fac,xp,xm,yp,ym) bind(C,name='dla_dense_lrprec2')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: fac, xp(*), xm(*), yp(*), ym(*)
    end subroutine
    subroutine dla_last_solve_info(iters,matvec_cols,restarts) bind(C,name='dla_last_solve_info')
      import :: c_int
      integer(c_int) :: iters, matvec_cols, restarts
    end subroutine
  end interface
  integer, parameter  :: n = 300, n_want = 4, n_eig = 8, itmax = 100, m_max = 20
  integer(c_int), parameter :: pair_ab = 0, pair_sd = 1      ! DLA_DENSE_LR_PAIR_AB, DLA_DENSE_LR_PAIR_SD
  real(dp), parameter :: tol = 1.0e-9_dp
  integer  :: i, j
  logical  :: ok
  real(dp), allocatable :: a(:,:), b(:,:), s(:,:), d(:,:), w(:), xy(:,:), guess(:,:), lhs(:), rhs(:), vp(:), vm(:)
!
! the four matrices, as the caller holds them
!
  allocate (a(n,n), b(n,n), s(n,n), d(n,n))
  do j = 1, n
    do i = 1, n
      if (i.eq.j) then
        a(i,j) = real(i,dp) + 3.5_dp
        b(i,j) = 1.5_dp
        s(i,j) = 1.0_dp + 0.5_dp/real(1+mod(i,7),dp)
        d(i,j) = 0.0_dp
      else
        a(i,j) = 0.12_dp/real(i+j,dp)
        b(i,j) = 0.08_dp/real(i+j,dp)
        s(i,j) = 0.01_dp*cos(real(i+j,dp))/real(1+abs(i-j),dp)
        d(i,j) = 0.02_dp*sin(0.3_dp*real(i+j,dp))/real(1+abs(i-j),dp)
        if (j.lt.i) d(i,j) = -d(i,j)
      end if
    end do
  end do
  if (dla_dense_setup_lr_pair(dla_default_ctx(), pair_ab, n, a, n, b, n).ne.0) stop 'A, B setup failed'
  if (dla_dense_setup_lr_pair(dla_default_ctx(), pair_sd, n, s, n, d, n).ne.0) stop 'S, D setup failed'
  call diaglib_amd_config(callbacks_on_device=.true., evec_on_device=.false.)
!
  allocate (w(n_eig), xy(2*n,n_eig), guess(2*n,n_eig), lhs(2*n), rhs(2*n), vp(n), vm(n))
!
! guess: that of examples/fortran_sparse_lr_caller, sin(0.37 i j + j) concentrated on the first 40 rows
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
  call caslr_eff_driver(.false.,n,2*n,n_want,n_eig,itmax,tol,m_max,dla_dense_apbmul,dla_dense_ambmul,dla_dense_spdmul, &
                        dla_dense_smdmul,dla_dense_lrprec2,w,xy,ok)
  call report('DENSE CASLR_EFF')
!
! ... and the traditional one on the same matrices
!
  xy = guess
  call caslr_driver(.false.,n,2*n,n_want,n_eig,itmax,tol,m_max,dla_dense_apbmul,dla_dense_ambmul,dla_dense_spdmul, &
                    dla_dense_smdmul,dla_dense_lrprec1,w,xy,ok)
  call report('DENSE CASLR')
  if (dla_dense_drop_lr(dla_default_ctx()).ne.0) stop 'drop failed'
  call diaglib_amd_config(release_cache=.true.)
!
contains
!
! the caller's own check, from its arrays on the host: with v+ = Y + Z, v- = Y - Z the pencil reads
!   (A+B) v+ = w (S-D) v-   and   (A-B) v- = w (S+D) v+      (reference diaglib.f90:1027-1046)
!
  subroutine report(tag)
    character(len=*), intent(in) :: tag
    integer(c_int) :: iters, cols, restarts
    real(dp)       :: resmax
    integer        :: c
    call dla_last_solve_info(iters, cols, restarts)
    resmax = 0.0_dp
    do c = 1, n_want
      vp = xy(1:n,c) + xy(n+1:2*n,c)
      vm = xy(1:n,c) - xy(n+1:2*n,c)
      lhs(1:n)     = matmul(a + b, vp)
      rhs(1:n)     = matmul(s - d, vm)
      lhs(n+1:2*n) = matmul(a - b, vm)
      rhs(n+1:2*n) = matmul(s + d, vp)
      resmax = max(resmax, sqrt(sum((lhs - w(c)*rhs)**2))/sqrt(sum(lhs**2)))
    end do
    write(6,'(a,a,l2,i6)') tag, ' ok/iterations:', ok, iters
    write(6,'(a,a,4es24.15)') tag, ' eig:', w(1:n_want)
    write(6,'(a,a,es12.4)') tag, ' max residual:', resmax
  end subroutine report
end program dense_lr_caller
