#include "ca_device_types.h"
namespace ca3d
{
namespace jit
{
#include "ca_bitops.inc"
#include "ca_jit_rule.inc"
#include "ca_bitslice.inc"
#include "ca_packed_roll_kernel.inc"
}
}
