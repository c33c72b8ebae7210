!------------------------------------------------------------------------------
! conductivity_mod -- SHADOW of the reference's module of the same name (source/conductivity.f90), for the zero-edit drop-in build.
!
! The reference's conductivity.f90 is compiled unchanged under another module name (-Dconductivity_mod=conductivity_ref_mod),
! fortran/conductivity_gpu.f90 extends its type from there, and THIS module hands that extended type out under the reference's names:
! `type(conductivity) :: conductivity_obj ; conductivity_obj = conductivity(self_obj)` in calculation.f90:969,1067 then declares and
! constructs a conductivity_gpu.  Recipe: fortran/build_dropin.sh; INTEGRATION.md section 2.
!------------------------------------------------------------------------------
module conductivity_mod
   use conductivity_gpu_mod, only: conductivity => conductivity_gpu
   implicit none
   private
   public :: conductivity
end module conductivity_mod
