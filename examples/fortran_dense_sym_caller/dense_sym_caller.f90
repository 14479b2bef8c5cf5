!
! examples/fortran_dense_sym_caller/dense_sym_caller.f90 -- examples/fortran_dense_caller with the two SYMMETRIC matrices stored as
! one triangle each (include/diaglib_amd.h: dla_dense_setup_sym): about half the device memory, and a product that streams every
! stored byte once.
!
! The only lines that differ from the full-storage caller are the two set-up calls: the operator is handed over by its lower
! triangle (uplo = 'L'), the metric by its upper one ('U').  The other strict triangle of either array is never read -- here it
! holds -huge() to show it -- and dla_dense_matvec / dla_dense_precnd / dla_dense_bvec keep their names and shapes: the slot
! remembers how it is stored.  davidson_driver, lobpcg_driver and gen_david_driver are called through the unmodified module
! interface in device mode; the caller's own check uses the full arrays it keeps on the host.
!
! A: a_ii = i + 1, a_ij = 1/(i+j) (the harness' matrix).  B: b_ii = 1 + 0.25 sin^2(0.003 (i-1)), b_ij = 0.05/(i-j)^2 -- strictly
! diagonally dominant (off-diagonal row sums below 0.05 pi^2 / 3 = 0.165), hence positive definite.
!
program dense_sym_caller
  use real_precision
  use iso_c_binding
  use diaglib, only : davidson_driver, lobpcg_driver, gen_david_driver, diaglib_amd_config
  implicit none
  interface
    function dla_default_ctx() bind(C,name='dla_default_ctx') result(ctx)
      import :: c_ptr
      type(c_ptr) :: ctx
    end function
    function dla_dense_setup_sym(ctx,which,n,a,lda,uplo) bind(C,name='dla_dense_setup_sym') result(st)
      import :: c_ptr, c_int, c_double, c_char
      type(c_ptr), value    :: ctx
      integer(c_int), value :: which, n, lda
      real(c_double)        :: a(lda,*)
      character(kind=c_char), value :: uplo
      integer(c_int)        :: st
    end function
    subroutine dla_dense_matvec(n,m,x,ax) bind(C,name='dla_dense_matvec')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), ax(*)
    end subroutine
    subroutine dla_dense_bvec(n,m,x,bx) bind(C,name='dla_dense_bvec')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), bx(*)
    end subroutine
    subroutine dla_dense_precnd(n,m,fac,x,px) bind(C,name='dla_dense_precnd')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: fac, x(*), px(*)
    end subroutine
    subroutine dla_last_solve_info(iters,matvec_cols,restarts) bind(C,name='dla_last_solve_info')
      import :: c_int
      integer(c_int) :: iters, matvec_cols, restarts
    end subroutine
  end interface
  integer, parameter  :: n = 1000, n_want = 6, itmax = 300, m_max = 20
  real(dp), parameter :: tol = 1.0e-9_dp
  integer  :: n_eig, i, j
  logical  :: ok
  real(dp), allocatable :: a(:,:), b(:,:), al(:,:), bu(:,:), eig(:), evec(:,:), guess(:,:)
!
! the two matrices, as a harness-style caller holds them (a, b: kept for the check), and what is handed over: the lower triangle
! of a in al, the upper triangle of b in bu, the other strict triangle of each filled with -huge()
!
  allocate (a(n,n), b(n,n), al(n,n), bu(n,n))
  do j = 1, n
    do i = 1, n
      if (i.eq.j) then
        a(i,j) = real(i+1,dp)
        b(i,j) = 1.0_dp + 0.25_dp*sin(0.003_dp*real(i-1,dp))**2
      else
        a(i,j) = 1.0_dp/real(i+j,dp)
        b(i,j) = 0.05_dp/real(i-j,dp)**2
      end if
    end do
  end do
  al = -huge(1.0_dp)
  bu = -huge(1.0_dp)
  do j = 1, n
    al(j:n,j) = a(j:n,j)
    bu(1:j,j) = b(1:j,j)
  end do
  if (dla_dense_setup_sym(dla_default_ctx(), 0_c_int, n, al, n, 'L').ne.0) stop 'operator setup failed'
  if (dla_dense_setup_sym(dla_default_ctx(), 1_c_int, n, bu, n, 'U').ne.0) stop 'metric setup failed'
  deallocate (al, bu)
  call diaglib_amd_config(callbacks_on_device=.true., evec_on_device=.false.)
!
  n_eig = min(2*n_want, n_want+5)
  allocate (eig(n_eig), evec(n,n_eig), guess(n,n_eig))
  guess = 0.0_dp
  do i = 1, n_eig
    guess(i,i) = 1.0_dp
  end do
!
! Davidson-Liu and LOBPCG on A x = lambda x (callers of the reference: main.f90:318-400)
!
  evec = guess
  call davidson_driver(.false.,n,n_want,n_eig,itmax,tol,m_max,0.0_dp,dla_dense_matvec,dla_dense_precnd,eig,evec,ok)
  call report('DENSE SYM DAVIDSON', .false.)
  evec = guess
  call lobpcg_driver(.false.,.false.,n,n_want,n_eig,itmax,tol,0.0_dp,dla_dense_matvec,dla_dense_precnd,dla_dense_bvec,eig,evec,ok)
  call report('DENSE SYM LOBPCG', .false.)
!
! Davidson-Liu with the metric, A x = lambda B x (main.f90:403-526)
!
  evec = guess
  call gen_david_driver(.false.,n,n_want,n_eig,itmax,tol,m_max,0.0_dp,dla_dense_matvec,dla_dense_precnd,dla_dense_bvec,eig,evec,ok)
  call report('DENSE SYM GEN_DAVIDSON', .true.)
  call diaglib_amd_config(release_cache=.true.)
!
contains
!
! the caller's own check, from its arrays on the host: || A x - eig B x || and x^T B x (B = I without the metric)
!
  subroutine report(tag, gen)
    character(len=*), intent(in) :: tag
    logical, intent(in)          :: gen
    integer(c_int) :: iters, cols, restarts
    real(dp)       :: resmax, orth
    real(dp), allocatable :: ax(:,:), bx(:,:)
    integer        :: c
    call dla_last_solve_info(iters, cols, restarts)
    allocate (ax(n,n_want), bx(n,n_want))
    ax = matmul(a, evec(:,1:n_want))
    if (gen) then
      bx = matmul(b, evec(:,1:n_want))
    else
      bx = evec(:,1:n_want)
    end if
    resmax = 0.0_dp
    orth = 0.0_dp
    do c = 1, n_want
      resmax = max(resmax, sqrt(sum((ax(:,c) - eig(c)*bx(:,c))**2)))
      orth = max(orth, abs(dot_product(evec(:,c), bx(:,c)) - 1.0_dp))
    end do
    write(6,'(a,a,l2,i6)') tag, ' ok/iterations:', ok, iters
    write(6,'(a,a,6es24.15)') tag, ' eig:', eig(1:n_want)
    write(6,'(a,a,2es12.4)') tag, ' max residual, max |x^T B x - 1|:', resmax, orth
  end subroutine report
end program dense_sym_caller
