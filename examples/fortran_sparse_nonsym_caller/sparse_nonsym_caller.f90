!
! examples/fortran_sparse_nonsym_caller/sparse_nonsym_caller.f90 -- a Fortran caller of nonsym_driver whose SPARSE non-symmetric
! matrix lives on the device once.
!
! The matrix has a known real spectrum: A = D S D^-1 with S symmetric and banded -- s_ii = i + 1, s_ij = 1/(i + j) for
! |i - j| in {1, 2, 17} (1-based) -- and D = diag(exp(t_i)), t_i = 0.01 sin(1.3 i).  So a_ij = exp(t_i - t_j) s_ij, the pattern is the
! band, and the eigenvalues are those of S.  The CSR arrays are handed over once (dla_spmm_setup_csr_fmt), the transposed index is
! prepared (dla_spmm_transpose_prepare), the driver is switched to device callbacks, and dla_spmm_matvec / dla_spmm_matvec_t /
! dla_spmm_precnd go where the harness' mmult / mmult_l / mprec went (main.f90:72-171): the transposed product fetches the values
! of the one stored copy, so nothing is stored twice.  nonsym_driver is called through the module interface with side = 'c'; the
! caller prints what examples/fortran_nonsym_caller prints.
!
!   sparse_nonsym_caller [n [host]]     n: default 300; host: the same solve with host callbacks on the CSR arrays, for timing
!
module sparse_nonsym_host
!
! the caller's CSR arrays (0-based, as the library takes them) and its host callbacks
!
  use real_precision
  use iso_c_binding
  implicit none
  integer(c_long_long), allocatable :: rowptr(:)
  integer(c_int), allocatable       :: colind(:)
  real(c_double), allocatable       :: values(:), diag(:)
contains
  subroutine mmult(nn,m,x,ax)
    integer,  intent(in)    :: nn, m
    real(dp), intent(in)    :: x(nn,m)
    real(dp), intent(inout) :: ax(nn,m)
    integer :: r, c
    integer(c_long_long) :: p
    ax = 0.0_dp
    do c = 1, m
      do r = 1, nn
        do p = rowptr(r) + 1, rowptr(r+1)
          ax(r,c) = ax(r,c) + values(p)*x(colind(p)+1,c)
        end do
      end do
    end do
  end subroutine mmult
!
  subroutine mmult_l(nn,m,x,ax)
    integer,  intent(in)    :: nn, m
    real(dp), intent(in)    :: x(nn,m)
    real(dp), intent(inout) :: ax(nn,m)
    integer :: r, c
    integer(c_long_long) :: p
    ax = 0.0_dp
    do c = 1, m
      do r = 1, nn
        do p = rowptr(r) + 1, rowptr(r+1)
          ax(colind(p)+1,c) = ax(colind(p)+1,c) + values(p)*x(r,c)
        end do
      end do
    end do
  end subroutine mmult_l
!
  subroutine mprec(nn,m,fac,x,px)
    integer,  intent(in)    :: nn, m
    real(dp), intent(in)    :: fac, x(nn,m)
    real(dp), intent(inout) :: px(nn,m)
    integer :: r, c
    do c = 1, m
      do r = 1, nn
        if (abs(diag(r)+fac).gt.1.0e-5_dp) then
          px(r,c) = x(r,c)/(diag(r) + fac)
        else
          px(r,c) = x(r,c)
        end if
      end do
    end do
  end subroutine mprec
end module sparse_nonsym_host
!
program sparse_nonsym_caller
  use real_precision
  use iso_c_binding
  use sparse_nonsym_host
  use diaglib, only : nonsym_driver, diaglib_amd_config
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
    function dla_spmm_transpose_prepare(ctx,fmt) bind(C,name='dla_spmm_transpose_prepare') result(st)
      import :: c_ptr, c_int
      type(c_ptr), value    :: ctx
      integer(c_int), value :: fmt
      integer(c_int)        :: st
    end function
    subroutine dla_spmm_matvec(n,m,x,ax) bind(C,name='dla_spmm_matvec')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), ax(*)
    end subroutine
    subroutine dla_spmm_matvec_t(n,m,x,y) bind(C,name='dla_spmm_matvec_t')
      import :: c_int, c_double
      integer(c_int) :: n, m
      real(c_double) :: x(*), y(*)
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
  integer, parameter  :: n_want = 4, n_eig = 8, itmax = 200, m_max = 10
  integer, parameter  :: offsets(7) = (/ -17, -2, -1, 0, 1, 2, 17 /)
  integer(c_int), parameter :: fmt_auto = 2
  real(dp), parameter :: tol = 1.0e-9_dp
  integer  :: n, i, j, k
  logical  :: ok, on_host
  character(len=32) :: arg
  real(dp) :: sij, biorth
  integer(8) :: c0, c1, rate
  integer(c_long_long) :: nnz
  integer(c_int) :: iters, cols, restarts
  real(dp), allocatable :: eig(:), evec_r(:,:), evec_l(:,:), small(:,:)
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
! the matrix in CSR form, columns ascending inside every row
!
  allocate (rowptr(n+1), colind(7*n), values(7*n), diag(n))
  nnz = 0
  rowptr(1) = 0
  do i = 1, n
    do k = 1, 7
      j = i + offsets(k)
      if (j.lt.1 .or. j.gt.n) cycle
      if (i.eq.j) then
        sij = real(i+1,dp)
        diag(i) = sij
      else
        sij = 1.0_dp/real(i+j,dp)
      end if
      nnz = nnz + 1
      colind(nnz) = j - 1
      values(nnz) = exp(t_of(i) - t_of(j))*sij
    end do
    rowptr(i+1) = nnz
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
    call nonsym_driver(.false.,n,n_want,n_eig,itmax,tol,m_max,0.0_dp,mmult,mmult_l,mprec,eig,evec_r,evec_l,'c',ok)
  else
    if (dla_spmm_setup_csr_fmt(dla_default_ctx(), n, rowptr, colind, values, fmt_auto).ne.0) stop 'operator setup failed'
    if (dla_spmm_transpose_prepare(dla_default_ctx(), fmt_auto).ne.0) stop 'transposed index failed'
    call diaglib_amd_config(callbacks_on_device=.true., evec_on_device=.false.)
    call nonsym_driver(.false.,n,n_want,n_eig,itmax,tol,m_max,0.0_dp,dla_spmm_matvec,dla_spmm_matvec_t,dla_spmm_precnd, &
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
! the exponent of the diagonal similarity transform, |t_i| <= 0.01
!
  function t_of(r) result(t)
    integer, intent(in) :: r
    real(dp) :: t
    t = 0.01_dp*sin(1.3_dp*real(r,dp))
  end function t_of
end program sparse_nonsym_caller
