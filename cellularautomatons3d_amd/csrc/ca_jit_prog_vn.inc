namespace ca3d_jit
{
#include "ca_bitops.inc"
#include "ca_packed_vn_kernel.inc"
}
