// launch_group_measure_u16.hip -- see launch_group_encode.inc: the measuring form for samples of 9 to 16 bits.  Compiled for gfx950 only.
#define JLS_UNIT_WIDE 1
#define JLS_UNIT_MEASURE 1
#include "launch_group_encode.inc"
