// launch_group_encode_u8.hip -- see launch_group_encode.inc: the encoding form for samples of up to 8 bits.  Compiled for gfx950 only.
#define JLS_UNIT_WIDE 0
#define JLS_UNIT_MEASURE 0
#include "launch_group_encode.inc"
