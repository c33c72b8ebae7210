!------------------------------------------------------------------------------
! exchange_mod -- SHADOW of the reference's module of the same name (source/exchange.f90), for the zero-edit drop-in build.
!
! The reference's exchange.f90 is compiled unchanged under another module name (-Dexchange_mod=exchange_ref_mod),
! fortran/exchange_gpu.f90 extends its type from there, and THIS module hands that extended type out under the reference's names:
! `type(exchange), target :: exchange_obj ; exchange_obj = exchange(bands_obj)` in calculation.f90:830,923 then declares and
! constructs an exchange_gpu.  Recipe: fortran/build_dropin.sh; INTEGRATION.md section 2.
!------------------------------------------------------------------------------
module exchange_mod
   use exchange_gpu_mod, only: exchange => exchange_gpu
   implicit none
   private
   public :: exchange
end module exchange_mod
