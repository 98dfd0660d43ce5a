// launch_group_measure_u8.hip -- see launch_group_encode.inc: the measuring form for samples of up to 8 bits.  Compiled for gfx950 only.
#define JLS_UNIT_WIDE 0
#define JLS_UNIT_MEASURE 1
#include "launch_group_encode.inc"
