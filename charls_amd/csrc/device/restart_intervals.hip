// restart_intervals.hip -- both halves of restart_intervals.h, for a unit that wants the decode and the encode kernels together
// (the CPU emulator, tests/emu/emu_driver.cpp).  The library's launch units include one half each: decode_launch.hip
// restart_intervals_decode.hip, encode_launch.hip restart_intervals_encode.hip.
#pragma once
#include "restart_intervals_decode.hip"
#include "restart_intervals_encode.hip"
