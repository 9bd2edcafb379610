namespace ca3d_jit
{
#include "ca_bitops.inc"
#include "ca_resident_kernel.inc"
}
