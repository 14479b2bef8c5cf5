!
! examples/fortran_nonsym_caller/nonsym_caller.f90 -- a Fortran caller of nonsym_driver whose matrix lives on the device ONCE.
!
! The reference's harness exercises nonsym_driver on a dense matrix (main.f90:910-1178; matrix 4: the usual test matrix
! a_ii = i + 1, a_ij = 1/(i+j) under a similarity transform exp(-T) A exp(T) with ||T||_F = 0.01) and keeps a second array
! a_t = transpose(a) for the left product.  Here the array is handed over once (dla_dense_setup), the driver is switched to device
! callbacks, and dla_dense_matvec / dla_dense_matvec_t / dla_dense_precnd go where mmult / mmult_l / mprec went: the transposed
! product reads the same stored copy, so nothing is stored twice.  nonsym_driver is called through the module interface with
! side = 'c'; the caller then prints what it got: the eigenvalues and max |L^T R - I| (after 'c' the columns are biorthonormal
! bases of the two subspaces, not individual eigenvectors).
!
! T here is of rank one, T = alpha u v^T with u_i = sin(1.3 i), v_j = cos(0.7 j), so that exp(+-T) = I +- alpha phi(+-s) u v^T,
! s = alpha v^T u, phi(s) = (e^s - 1)/s, and the transform costs O(n^2) at any n (the harness sums a matrix exponential series).
!
!   nonsym_caller [n [host]]        n: default 300; host: the same solve with host callbacks on a and transpose(a), for timing
!
module nonsym_host
!
! the caller's arrays and its host callbacks (the harness' mmult, mmult_l and mprec, main.f90:72-171), for the timing run
!
  use real_precision
  implicit none
  real(dp), allocatable :: a(:,:), a_t(:,:)
contains
  subroutine mmult(nn,m,x,ax)
    integer,  intent(in)    :: nn, m
    real(dp), intent(in)    :: x(nn,m)
    real(dp), intent(inout) :: ax(nn,m)
    ax = matmul(a, x)
  end subroutine mmult
!
  subroutine mmult_l(nn,m,x,ax)
    integer,  intent(in)    :: nn, m
    real(dp), intent(in)    :: x(nn,m)
    real(dp), intent(inout) :: ax(nn,m)
    ax = matmul(a_t, x)
  end subroutine mmult_l
!
  subroutine mprec(nn,m,fac,x,px)
    integer,  intent(in)    :: nn, m
    real(dp), intent(in)    :: fac, x(nn,m)
    real(dp), intent(inout) :: px(nn,m)
    integer :: r, c
    do c = 1, m
      do r = 1, nn
        if (abs(a(r,r)+fac).gt.1.0e-5_dp) then
          px(r,c) = x(r,c)/(a(r,r) + fac)
        else
          px(r,c) = x(r,c)
        end if
      end do
    end do
  end subroutine mprec
end module nonsym_host
!
program nonsym_caller
  use real_precision
  use iso_c_binding
  use nonsym_host
  use diaglib, only : nonsym_driver, diaglib_amd_config
  implicit none
  interface
    function dla_default_ctx() bind(C,name='dla_default_ctx') result(ctx)
      import :: c_ptr
      type(c_ptr) :: ctx
    end function
    function dla_dense_setup(ctx,which,n,a,lda) bind(C,name='dla_dense_setup') result(st)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value    :: ctx
      integer(c_int), value :: which, n, lda
      real(c_double)        :: a(lda,*)
      integer(c_int)        :: st
    end function
    subroutine dla_dense_matvec(n,m,x,ax) bind(C,name='dla_dense_matvec')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), ax(*)
    end subroutine
    subroutine dla_dense_matvec_t(n,m,x,y) bind(C,name='dla_dense_matvec_t')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), y(*)
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
  integer, parameter  :: n_want = 4, n_eig = 8, itmax = 200, m_max = 10
  real(dp), parameter :: tol = 1.0e-9_dp
  integer  :: n, i, j
  logical  :: ok, on_host
  character(len=32) :: arg
  real(dp) :: alpha, s, cp, cm, vau, biorth
  integer(8) :: c0, c1, rate
  integer(c_int) :: iters, cols, restarts
  real(dp), allocatable :: u(:), v(:), au(:), va(:), eig(:), evec_r(:,:), evec_l(:,:), small(:,:)
!
  n = 300
  on_host = .false.
  if (command_argument_count().ge.1) then
    call get_command_argument(1, arg)
    read(arg,*) n
  end if
  if (command_argument_count().ge.2) then
    call get_command_argument(2, arg)
    on_host = trim(arg).eq.'host'
  end if
!
! the matrix, as a harness-style caller holds it
!
  allocate (a(n,n), u(n), v(n), au(n), va(n))
  do j = 1, n
    do i = 1, n
      if (i.eq.j) then
        a(i,j) = real(i+1,dp)
      else
        a(i,j) = 1.0_dp/real(i+j,dp)
      end if
    end do
    u(j) = sin(1.3_dp*real(j,dp))
    v(j) = cos(0.7_dp*real(j,dp))
  end do
  alpha = 0.01_dp/(sqrt(sum(u*u))*sqrt(sum(v*v)))
  s  = alpha*dot_product(v, u)
  cp = alpha*phi(s)
  cm = alpha*phi(-s)
  au  = matmul(a, u)
  va  = matmul(v, a)
  vau = dot_product(v, au)
  do j = 1, n
    do i = 1, n
      a(i,j) = a(i,j) + cp*au(i)*v(j) - cm*u(i)*va(j) - cm*cp*vau*u(i)*v(j)
    end do
  end do
!
  allocate (eig(n_eig), evec_r(n,n_eig), evec_l(n,n_eig))
  evec_r = 0.0_dp
  do i = 1, n_eig
    evec_r(i,i) = 1.0_dp
  end do
  evec_l = evec_r
  call system_clock(c0, rate)
  if (on_host) then
    allocate (a_t(n,n))
    a_t = transpose(a)
    call nonsym_driver(.false.,n,n_want,n_eig,itmax,tol,m_max,0.0_dp,mmult,mmult_l,mprec,eig,evec_r,evec_l,'c',ok)
  else
    if (dla_dense_setup(dla_default_ctx(), 0_c_int, n, a, n).ne.0) stop 'operator setup failed'
    call diaglib_amd_config(callbacks_on_device=.true., evec_on_device=.false.)
    call nonsym_driver(.false.,n,n_want,n_eig,itmax,tol,m_max,0.0_dp,dla_dense_matvec,dla_dense_matvec_t,dla_dense_precnd, &
                       eig,evec_r,evec_l,'c',ok)
  end if
  call system_clock(c1)
  call dla_last_solve_info(iters, cols, restarts)
!
! the caller's own check
!
  allocate (small(n_eig,n_eig))
  small = matmul(transpose(evec_l), evec_r)
  biorth = 0.0_dp
  do j = 1, n_eig
    do i = 1, n_eig
      biorth = max(biorth, abs(small(i,j) - merge(1.0_dp, 0.0_dp, i.eq.j)))
    end do
  end do
  write(6,'(a,l2,2i6)')     'NONSYM ok/iterations/matvec columns:', ok, iters, cols
  write(6,'(a,4es24.15)')   'NONSYM eig:', eig(1:n_want)
  write(6,'(a,es12.4)')     'NONSYM max |L^T R - I|:', biorth
  write(6,'(a,a,i7,f12.6)') 'NONSYM mode/n/seconds: ', merge('host  ', 'device', on_host), n, real(c1-c0,dp)/real(rate,dp)
  call diaglib_amd_config(release_cache=.true.)
!
contains
!
! (e^s - 1)/s by its series (|s| is of the order 1e-2 or below)
!
  function phi(x) result(p)
    real(dp), intent(in) :: x
    real(dp) :: p, term
    integer  :: k
    p = 1.0_dp
    term = 1.0_dp
    do k = 2, 14
      term = term*x/real(k,dp)
      p = p + term
    end do
  end function phi
end program nonsym_caller
