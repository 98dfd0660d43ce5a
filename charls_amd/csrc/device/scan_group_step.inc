// scan_group_step.inc -- the step loop of decode_scans_group (scan_group_decode.hip) written out for gfx950.
//
// The C++ rendering of the same loop is in scan_group_decode.hip (it is what the CPU harness runs and it is the specification:
// every name below is a variable there).  Reference semantics: one regular-mode sample per trip -- context id and sign
// (src/jpegls_algorithm.hpp:98-117,165-168), MED prediction (:143-161), the Golomb parameter (src/regular_mode_context.hpp:99-111),
// the limited-length code (src/scan_decoder_core.hpp:38-69), the error correction (src/regular_mode_context.hpp:36-42) and the
// update of A, B, C, N (:45-93).
//
// Why by hand: one wavefront of this instruction mix has its SIMD to itself and issues one instruction every 4.1 - 5 cycles
// (tools/microbench/issue_ceiling.hip), so a step costs its instruction count -- and, measured on the loop alone
// (tools/microbench/steploop.hip, profiles/r06_steploop_*), a few instructions cost many times that: a scalar branch on a
// mask a vector compare has just written (46 cycles for the RESET test of round 5's form), LDS stores that all 16 lanes of a
// scan issue to one address (34 + 20 cycles for the record and the sample).  So:
//   * ONE conditional branch per step.  Everything rare -- N had reached RESET (A.12's halving), run mode (Q = 0), a code the
//     loop does not take -- is one mask: the compare of N with RESET is issued as soon as the record is there, run mode reads
//     record 0, which no context uses and whose N the kernel presets to RESET, and the mask is looked at once, at the end.
//   * the store of the sample sits behind the request of the record, where nothing waits for it.
//   * the three LDS round trips of the chain are covered by independent work: Q3 <- gradient table [Rc - Ra] under the commit
//     of the previous step, the request of the bit window, the predictor and A.13 of the previous step; the context record
//     under bit window, unary prefix, sign and the prefix test; the prepared entry of the NEXT sample is requested in the
//     middle of a step, behind the last use of this step's.
//   * two steps per trip of the loop (a taken branch costs more than a not-taken one), and the trip is the unit of the count and
//     of the pointer advances (JLS_STEP_TRIP_COUNT, JLS_STEP_TRIP_POINTERS below).
// Lanes outside their line are switched off (EXEC) for the whole loop.
//
// Fixed registers (v80 - v127, s80 - s99 are clobbered; v80 - v92: the rare path; v93 = RESET; v94 - v99: near-lossless constants):
// v100 = 2912 (8 * 364), v101 = byte selector of v_perm, v102 = -cap
// (wide), v103 = 127, v104 = -128, v105 = 1; temporaries v108 - v117; pairs: E = v[118:119] / v[106:107] entry {Rc | T << 16, Rb} (8-bit containers: {Rc | Rb << 8 | T << 16, Rb - Rc}) of the
// two copies of the step,
// W = v[120:121] ring words, R = v[122:123] record {A, N | C << 8 | B << 16}, M = v[124:125] {window beyond the prefix, u},
// MM = v[126:127] = M << k (v127 = the mapped error).  s[92:93]: lanes whose N = RESET (or run mode); s[96:97]: lanes whose
// code the loop does not take; s[98:99]: EXEC of the caller.
//
// Hazards kept by hand (the assembler does not pad inline assembly): a VALU that reads an SGPR or a lane mask written by a VALU
// comes at least two wait states behind it (v_cmp -> v_cndmask, v_readlane -> v_cmp), a lane select of v_readlane four behind
// its write (tests/test_inline_asm_hazards_cpu.py audits both in the compiled kernels); LDS results are awaited by count (LDS
// operations complete in order).

#define JLS_SDWA(s0, s1) " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" s0 " src1_sel:" s1 "\n"

// MED relative to Ra, for samples in 8-bit containers (default on; -DJLS_STEP_MED_FROM_RA=0 for the A/B: every rendering then
// has the text of the wide one).  median(Ra, Rb, Ra + Rb - Rc) = Ra + median(0, Rb - Ra, Rb - Rc): with the prepared entry
// {Rc | Rb << 8 | T << 16, Rb - Rc} every reader of Ra in a step -- the Q3 difference, the two SDWA instructions of the predictor,
// the one-byte store -- takes its low byte, and the lossless step of a MAXVAL = 255 scan leaves the sample unmasked: one
// instruction less on the chain Ra -> Q3.  (VOP3 has no SDWA selects: v_med3 of the absolute form needs a clean Ra.)
#ifndef JLS_STEP_MED_FROM_RA
#define JLS_STEP_MED_FROM_RA 1
#endif

// The count of a call is a count of TRIPS (default on; -DJLS_STEP_TRIP_COUNT=0: a count of steps, tested behind every copy).
// The exit test stands once per trip, behind the last copy, and its branch is the back edge: one conditional branch taken per
// trip instead of a not-taken one per step and a taken s_branch.  A call of an odd number of steps enters the loop at copy "b"
// (L_enterb loads that copy's entry pair), so a line's last sample -- one step -- is one trip.  The run service brings the count
// down to whole trips from the copy it was called from (JLS_STEP_BUDGET_*), and leaves through L_doneb -- the state of a loop that
// ended by count -- when a served scan may not even finish the trip.
#ifndef JLS_STEP_TRIP_COUNT
#define JLS_STEP_TRIP_COUNT 1
#endif
// lm and pp advance once per trip (default on; -DJLS_STEP_TRIP_POINTERS=0: once per step).  Copy "b" adds both steps of the trip;
// copy "a" addresses through the offset fields of its DS instructions, so that between the place of a's advance and b's the true
// pointers are lm + SZ and pp + 8.  Whatever leaves the loop from copy "a" adds that on its way (L_donea, JLS_STEP_RARE_ENTER_A), and
// the run service works on true pointers and takes it off again when it returns into copy "a" (JLS_STEP_RARE_LEAVE_A).
#ifndef JLS_STEP_TRIP_POINTERS
#define JLS_STEP_TRIP_POINTERS 1
#endif
#if JLS_STEP_TRIP_POINTERS
#define JLS_STEP_ADVANCE_A(SZ) ""
#define JLS_STEP_ADVANCE_B(SZ) "v_add_u32 %[lm], 2 * " SZ ", %[lm]\n v_add_u32 %[pp], 16, %[pp]\n"
#define JLS_STEP_STORE_OFFSET_A(SZ) " offset:" SZ
#define JLS_STEP_NEXT_ENTRY_A "16"
#define JLS_STEP_TRUE_UP_A(SZ) "v_add_u32 %[lm], " SZ ", %[lm]\n v_add_u32 %[pp], 8, %[pp]\n"
#define JLS_STEP_RARE_ENTER_A(SZ) JLS_STEP_TRUE_UP_A(SZ)
#define JLS_STEP_RARE_LEAVE_A(SZ) "v_add_u32 %[lm], -" SZ ", %[lm]\n v_add_u32 %[pp], -8, %[pp]\n"
#else
#define JLS_STEP_ADVANCE_A(SZ) "v_add_u32 %[lm], " SZ ", %[lm]\n v_add_u32 %[pp], 8, %[pp]\n"
#define JLS_STEP_ADVANCE_B(SZ) JLS_STEP_ADVANCE_A(SZ)
#define JLS_STEP_STORE_OFFSET_A(SZ) ""
#define JLS_STEP_NEXT_ENTRY_A "8"
#define JLS_STEP_TRUE_UP_A(SZ) ""
#define JLS_STEP_RARE_ENTER_A(SZ) ""
#define JLS_STEP_RARE_LEAVE_A(SZ) ""
#endif
// how a copy ends: PER_STEP -- the count test of a loop that counts steps (DONE: its exit, NEXT: what follows when the loop goes on);
// with a count of trips copy "a" ends in nothing and copy "b" in the back edge
#define JLS_STEP_TAIL_PER_STEP(DONE, NEXT) "s_sub_u32 %[cnt], %[cnt], 1\n s_cbranch_scc1 " DONE "%=\n" NEXT
#if JLS_STEP_TRIP_COUNT
#define JLS_STEP_TAIL_A ""
#define JLS_STEP_TAIL_B "s_sub_u32 %[cnt], %[cnt], 1\n s_cbranch_scc0 L_stepa%=\n s_branch L_doneb%=\n"
// v89 = samples a served scan may still take -> trips it may still take behind this one; s[86:87] (copy "a"): scans that may not
// take the trip's second step
#define JLS_STEP_BUDGET_A "v_cmp_eq_u32_e64 s[86:87], 0, v89\n v_add_u32 v89, -1, v89\n v_lshrrev_b32 v89, 1, v89\n"
#define JLS_STEP_BUDGET_B "v_lshrrev_b32 v89, 1, v89\n"
#define JLS_STEP_SHORT_A "s_cmp_lg_u64 s[86:87], 0\n s_cbranch_scc1 L_doneb%=\n"   /* (lm and pp are true here) */
#else
#define JLS_STEP_TAIL_A JLS_STEP_TAIL_PER_STEP("L_donea", "")
#define JLS_STEP_TAIL_B JLS_STEP_TAIL_PER_STEP("L_doneb", "s_branch L_stepa%=\n")
#define JLS_STEP_BUDGET_A ""
#define JLS_STEP_BUDGET_B ""
#define JLS_STEP_SHORT_A ""
#endif

#define JLS_STEP_PROLOGUE_CONSTANTS                                                                                                \
    "v_mov_b32 v100, 0xb60\n"                                                                                                     \
    "v_mov_b32 v101, 0x0c0c0400\n"                                                                                                \
    "v_mov_b32 v103, 0x7f\n"                                                                                                      \
    "v_mov_b32 v104, 0xffffff80\n"                                                                                                \
    "v_mov_b32 v105, 1\n"                                                                                                         \
    "v_mov_b32 v127, 0\n"                                                                                                         \
    "v_lshrrev_b32 v93, 16, %[cfg]\n"                                       /* RESET */                                          \
    "s_waitcnt lgkmcnt(0)\n"
// a loop that counts steps: every call starts at copy "a"
#define JLS_STEP_PROLOGUE_PER_STEP                                                                                                 \
    "s_mov_b64 s[98:99], exec\n"                                                                                                  \
    "s_mov_b64 exec, %[inl]\n"                                                                                                    \
    "ds_read_b64 v[118:119], %[pp] offset:8\n"                                                                                    \
    JLS_STEP_PROLOGUE_CONSTANTS
#if JLS_STEP_TRIP_COUNT
// cnt comes in as steps - 1: (steps - 1) >> 1 trips behind the first one, which is the second half of a trip when steps is odd
#define JLS_STEP_PROLOGUE                                                                                                          \
    "s_mov_b64 s[98:99], exec\n"                                                                                                  \
    "s_mov_b64 exec, %[inl]\n"                                                                                                    \
    "s_and_b32 s80, %[cnt], 1\n"                                                                                                  \
    "s_lshr_b32 %[cnt], %[cnt], 1\n"                                                                                              \
    "s_cmp_eq_u32 s80, 0\n"                                                                                                       \
    "s_cbranch_scc1 L_enterb%=\n"                                                                                                 \
    "ds_read_b64 v[118:119], %[pp] offset:8\n"                                                                                    \
    JLS_STEP_PROLOGUE_CONSTANTS
#define JLS_STEP_ENTER_B(SZ)                                                                                                       \
    "L_enterb%=:\n"                                                                                                               \
    "ds_read_b64 v[106:107], %[pp] offset:8\n"                                                                                    \
    JLS_STEP_RARE_LEAVE_A(SZ)                                               /* (copy "b" advances by the whole trip) */          \
    JLS_STEP_PROLOGUE_CONSTANTS                                                                                                    \
    "s_branch L_stepb%=\n"
#else
#define JLS_STEP_PROLOGUE JLS_STEP_PROLOGUE_PER_STEP
#define JLS_STEP_ENTER_B(SZ) ""
#endif

// The stores of a step: the previous step's record -- before this step's record is requested: it may be the same one -- and
// the previous step's sample, which nobody reads before the loop is over: it goes behind the request of the record, off the
// chain (LATE), or with the record (EARLY; the microbenchmark's comparison).  Both are issued by all lanes of a scan (the same
// value to the same address): narrowing EXEC to one lane per scan around them costs more than it saves
// (profiles/r06_steploop_v2_compositions.txt).
// (OFF: the offset field of the sample's store, JLS_STEP_STORE_OFFSET_A in copy "a")
#define JLS_STEP_STORES_LATE(ST, OFF) "ds_write2_b32 %[where], %[ua], v111 offset1:1\n", "2", ST " %[lm], %[a]" OFF "\n", "1"
#define JLS_STEP_STORES_EARLY(ST, OFF) "ds_write2_b32 %[where], %[ua], v111 offset1:1\n" ST " %[lm], %[a]" OFF "\n", "3", "", "0"

// The part of a step between the request of Q3 and its arrival, in three pieces: the order in which they are issued is a
// parameter (measured: tools/microbench/steploop.hip).
#define JLS_STEP_COMMIT_AND_WINDOW(SZ, TOP_EXTRA) \
    /* the previous step becomes final: bit position, and (TOP_EXTRA begins with the copy's JLS_STEP_ADVANCE_*) line slot, entry */ \
    "v_add3_u32 %[p], %[p], %[u1], %[k]\n" \
    TOP_EXTRA \
    "v_bfe_u32 v109, %[p], 5, 8\n" \
    "v_lshl_add_u32 v109, v109, 2, %[ring]\n" \
    "ds_read2_b32 v[120:121], v109 offset1:1\n"                             /* LDS 2 */
#define JLS_STEP_PREDICTOR(RC, E0, E1) \
    /* MED predictor = median(Ra, Rb, Ra + Rb - Rc) */ \
    "v_add_u32 v115, %[a], " E1 "\n" \
    "v_sub_u32_sdwa v115, v115, " E0 JLS_SDWA("DWORD", RC) \
    "v_med3_i32 v115, v115, %[a], " E1 "\n"
// the same number from the entry {Rc | Rb << 8 | T << 16, Rb - Rc}: Ra + median(0, Rb - Ra, Rb - Rc), Ra by its low byte
#define JLS_STEP_PREDICTOR_FROM_RA(RC, E0, E1) \
    "v_sub_u32_sdwa v115, " E0 ", %[a]" JLS_SDWA("BYTE_1", "BYTE_0") \
    "v_med3_i32 v115, v115, 0, " E1 "\n" \
    "v_add_u32_sdwa v115, v115, %[a]" JLS_SDWA("DWORD", "BYTE_0")
#define JLS_STEP_A13 \
    /* A.13 of the previous step: minus_delta = 1 - (tb > 0) - (tb + N' > 0), B' = med3(tb + minus_delta N', 1 - N', 0), C' */ \
    "v_med3_i32 v110, %[utb], 0, 1\n" \
    "v_add_u32 v111, %[utb], %[un1]\n" \
    "v_med3_i32 v111, v111, 0, 1\n" \
    "v_add_u32 v110, v110, v111\n" \
    "v_sub_u32 v110, 1, v110\n" \
    "v_sub_u32 v111, %[cc], v110\n" \
    "v_mad_i32_i24 v112, v110, %[un1], %[utb]\n" \
    "v_med3_i32 v111, v111, v104, v103\n" \
    "v_sub_u32 v113, 1, %[un1]\n" \
    "v_med3_i32 v112, v112, v113, 0\n" \
    "v_perm_b32 v111, v111, %[un1], v101\n" \
    "v_lshl_or_b32 v111, v112, 16, v111\n"

// What differs between lossless and near-lossless scans (four arguments of a step: what follows the sign of the context, the
// low bit of the mapped error, the reconstruction, the register B is updated from).
//  * lossless: odd is flipped when k = 0 and 2 B + N - 1 < 0 (src/regular_mode_context.hpp:36-42); the sample is
//    (Px + sign Errval) mod 2^bpp; B += Errval.
//  * near-lossless (src/default_traits.hpp:83-87,172-184): no correction; Rx = Px + sign Errval (2 NEAR + 1), brought back
//    into -NEAR .. MAXVAL + NEAR by RANGE (2 NEAR + 1) and clamped; B += Errval (2 NEAR + 1).  v94 = 2 NEAR + 1, v95 = -v94,
//    v96 = -NEAR, v97 = MAXVAL + NEAR, v98 = RANGE (2 NEAR + 1), v99 = -v98; v117 = sign (2 NEAR + 1), v112 = Errval (2 NEAR + 1).
#define JLS_STEP_ODD_LOSSLESS                                                                                                      \
    "v_add_u32_sdwa v109, v123, sext(v123)" JLS_SDWA("BYTE_0", "WORD_1")                                                          \
    "v_add_u32_sdwa v109, v109, sext(v123)" JLS_SDWA("DWORD", "WORD_1")                                                           \
    "v_add_u32 v109, -1, v109\n"                                                                                                  \
    "v_add_u32 v110, -1, %[k]\n"                                                                                                  \
    "v_and_b32 v109, v109, v110\n"                                                                                                \
    "v_lshrrev_b32 v109, 31, v109\n"                                                                                              \
    "v_bitop3_b32 v109, v127, 1, v109 bitop3:0x48\n"
#define JLS_STEP_RECON_LOSSLESS                                                                                                    \
    "v_mad_i32_i24 v115, v111, v116, v115\n"                                                                                      \
    "v_and_b32 %[a], %[smax], v115\n"
#define JLS_STEP_LOSSLESS "", JLS_STEP_ODD_LOSSLESS, JLS_STEP_RECON_LOSSLESS, "v111"
// MAXVAL = 255 with MED relative to Ra: the sample is the low byte of Px + sign Errval; nothing in the loop reads more of it, and
// the code behind the loop gets it masked (JLS_STEP_EXIT_BYTE)
#define JLS_STEP_RECON_LOSSLESS_BYTE "v_mad_i32_i24 %[a], v111, v116, v115\n"
#define JLS_STEP_LOSSLESS_BYTE "", JLS_STEP_ODD_LOSSLESS, JLS_STEP_RECON_LOSSLESS_BYTE, "v111"
#define JLS_STEP_EXIT_BYTE "v_and_b32 %[a], 0xff, %[a]\n"
#define JLS_STEP_RECON_NEAR                                                                                                        \
    "v_mad_i32_i24 v115, v111, v117, v115\n"                                                                                      \
    "v_cmp_lt_i32 vcc, v115, v96\n"                                                                                               \
    "v_cmp_gt_i32 s[88:89], v115, v97\n"                                                                                          \
    "v_mul_i32_i24 v112, v111, v94\n"                                                                                             \
    "v_cndmask_b32 v113, 0, v98, vcc\n"                                                                                           \
    "v_cndmask_b32_e64 v113, v113, v99, s[88:89]\n"                                                                               \
    "v_add_u32 v115, v115, v113\n"                                                                                                \
    "v_med3_i32 %[a], v115, 0, %[smax]\n"
#define JLS_STEP_NEAR "v_cndmask_b32 v117, v94, v95, vcc\n", "v_and_b32 v109, 1, v127\n", JLS_STEP_RECON_NEAR, "v112"
#define JLS_STEP_NEAR_CONSTANTS                                                                                                    \
    "s_and_b32 s80, %[nr], 0xff\n"                                          /* NEAR */                                           \
    "s_lshr_b32 s81, %[nr], 8\n"                                            /* RANGE (2 NEAR + 1) */                             \
    "v_lshl_add_u32 v94, s80, 1, 1\n"                                                                                             \
    "v_sub_u32 v96, 0, s80\n"                                                                                                     \
    "v_mov_b32 v98, s81\n"                                                                                                        \
    "v_sub_u32 v95, 0, v94\n"                                                                                                     \
    "v_sub_u32 v97, %[smax], v96\n"                                                                                               \
    "v_sub_u32 v99, 0, v98\n"

// One step.  SFX: label suffix of this copy; TAIL: how the copy ends (JLS_STEP_TAIL_*); NEXT_OFFSET: the offset field of the request of
// the next entry ("8", JLS_STEP_NEXT_ENTRY_A in copy "a").
// RC: the half of the entry's first word that holds Rc ("BYTE_0" / "WORD_0"); ASEL: what the Q3 difference reads of Ra ("BYTE_0"
// with MED relative to Ra, else "DWORD"); PRED (an argument of ORDER): the predictor, JLS_STEP_PREDICTOR or _FROM_RA; SZ: bytes per sample; STORES: one of the above
// (four arguments: the early stores, the LDS operations that may be outstanding when Q3 is awaited, the late store, those that
// may be outstanding when the record is awaited);
// Q3_ADDR: from v108 = Rc - Ra to the table index in v108 (8-bit: nothing, the constant goes into the offset field);
// Q3_OFFSET: that offset; TOP_EXTRA / K_EXTRA / A_EXTRA: what wider samples add; KSEEN: the accumulation of k
// (invoked from inside another macro with STORES as ONE argument there: it has become four by the time this one is looked at)
#define JLS_STEP_BODY(SFX, TAIL, E0, E1, ENEXT, NEXT_OFFSET, RC, ASEL, SZ, BETWEEN, RING_WAIT, AFTER_REQUEST, EARLY_STORES, Q3_WAIT, LATE_STORE, RECORD_WAIT, Q3_ADDR, Q3_OFFSET, TOP_EXTRA, K_EXTRA, A_EXTRA, KSEEN, SIGN_EXTRA, ODD, RECON, UTB_SRC) \
    "L_step" SFX "%=:\n"                                                                                                          \
    /* Q3: the one gradient that depends on the sample just decoded */                                                            \
    "v_sub_u32_sdwa v108, " E0 ", %[a]" JLS_SDWA(RC, ASEL)                                                                       \
    Q3_ADDR                                                                                                                       \
    "ds_read_u8 v114, v108" Q3_OFFSET "\n"                                  /* LDS 1 */                                          \
    BETWEEN                                                                                                                       \
    EARLY_STORES                                                            /* LDS 3 (, 4) */                                    \
    "s_waitcnt lgkmcnt(" Q3_WAIT ")\n"                                      /* Q3 is here */                                     \
    "v_add_u32_sdwa %[qsu], v114, " E0 JLS_SDWA("DWORD", "WORD_1")                                                                \
    "ds_read_b64 " ENEXT ", %[pp] offset:" NEXT_OFFSET "\n"                 /* the next sample's entry, into the other copy's pair */ \
    "v_sad_u32 %[where], %[qsu], v100, %[recbase]\n"                                                                              \
    "ds_read_b64 v[122:123], %[where]\n"                                    /* the context record */                             \
    LATE_STORE                                                                                                                    \
    AFTER_REQUEST                                                                                                                 \
    "v_cmp_gt_u32 vcc, v100, %[qsu]\n"                                                                                            \
    "s_waitcnt lgkmcnt(" RING_WAIT ")\n"                                    /* the ring words are here */                        \
    "v_alignbit_b32 %[win], v121, v120, %[p]\n"                                                                                   \
    "v_ffbl_b32 v125, %[win]\n"                                                                                                   \
    "v_cndmask_b32_e64 v116, 1, -1, vcc\n"                                  /* sign of the context */                            \
    SIGN_EXTRA                                                                                                                    \
    "v_add_u32 %[u1], 1, v125\n"                                                                                                  \
    "v_lshrrev_b32 v124, %[u1], %[win]\n"                                                                                         \
    "v_bfrev_b32 v124, v124\n"                                                                                                    \
    "v_cmp_ge_u32 s[96:97], v125, %[limitv]\n"                              /* escape code, long prefix, empty window */         \
    "s_waitcnt lgkmcnt(" RECORD_WAIT ")\n"                                  /* the record is here */                             \
    "v_cmp_eq_u32_sdwa s[92:93], v123, v93 src0_sel:BYTE_0 src1_sel:DWORD\n"        /* N = RESET; also record 0 = run mode */   \
    /* k = max(0, ceil((bits(A) - bits(N)) / 2^23)): the subtraction saturates at 0, which is the max */                        \
    "v_cvt_f32_u32 v108, v122\n"                                                                                                  \
    "v_cvt_f32_ubyte0 v109, v123\n"                                                                                               \
    "v_add_u32 v108, 0x7fffff, v108\n"                                                                                            \
    "v_sub_u32_e64 v108, v108, v109 clamp\n"                                                                                      \
    "v_lshrrev_b32 %[k], 23, v108\n"                                                                                              \
    "v_lshlrev_b64 v[126:127], %[k], v[124:125]\n"                          /* v127 = mapped error */                            \
    K_EXTRA                                                                                                                       \
    ODD                                                                     /* v109 = odd: the low bit of the mapped error */    \
    "v_bfe_u32 v110, v127, 1, 17\n"                                         /* half (17 bits: a lane that cannot decode must not fake an overflow of A) */ \
    "v_sub_u32 v111, 0, v109\n"                                                                                                   \
    "v_xor_b32 v111, v110, v111\n"                                          /* Errval */                                         \
    "v_bfe_i32 %[cc], v123, 8, 8\n"                                                                                               \
    "v_mad_i32_i24 v115, %[cc], v116, v115\n"                                                                                     \
    "v_med3_i32 v115, v115, 0, %[smax]\n"                                                                                         \
    RECON                                                                   /* the sample */                                     \
    /* A.12 of this step: A + |Errval|, N + 1, B + Errval */                                                                      \
    "v_add3_u32 %[ua], v122, v110, v109\n"                                                                                        \
    A_EXTRA                                                                                                                       \
    "v_add_u32_sdwa %[un1], v123, v105" JLS_SDWA("BYTE_0", "DWORD")                                                               \
    "v_add_u32_sdwa %[utb], " UTB_SRC ", sext(v123)" JLS_SDWA("DWORD", "WORD_1")                                                  \
    KSEEN                                                                                                                         \
    "s_or_b64 s[94:95], s[92:93], s[96:97]\n"                               /* anything rare in any lane? */                     \
    "s_cbranch_scc1 L_rare" SFX "%=\n"                                                                                            \
    "L_back" SFX "%=:\n"                                                                                                          \
    TAIL                                                                    /* are the steps of this call done? */               \

// What is rare: lanes of s[92:93] -- N had reached RESET: A + |Errval|, B + Errval and N are halved before N is incremented
// (src/regular_mode_context.hpp:56-63; harmless in a lane whose "record" was record 0, which is run mode) -- and lanes that
// could not decode their sample: s[96:97] (an unusual code: the loop ends) and those in run mode.  The halving comes first:
// the lanes that did decode keep what it leaves when the loop ends here.
//
// Run mode inside the loop (src/scan_decoder_impl.hpp:264-337, src/scan_decoder_core.hpp:72-100, src/run_mode_context.hpp).
// Handled outside the loop a run event costs the wavefront ~ 400 instructions (the rest of the loop's bookkeeping, the
// handler, the way back in); here ~ 150, under the EXEC mask of the lanes in run mode, for the events that are frequent: a run
// of at most G samples (the lanes of the scan fill it with ONE store) that is interrupted inside its line, with RUNindex <= 16
// after its complete blocks (there J = RUNindex >> 2 and the samples of r blocks are ((4 + (r & 3)) << (r >> 2)) - 4), all of
// whose bits -- the ones of the complete blocks, the zero, J bits, the code of the interruption sample -- lie in the 32-bit
// window the step was given (it consumed nothing).  Ra and Rb come from the line (the step's store of Ra is behind it), both run
// contexts are read ahead of knowing which.  A lane that is served looks like one that decoded a regular sample at the end of its
// run: a = the interruption sample, u1 = the bits of the event, k = 0, its "context update" goes to the unused record 365, its
// line and entry pointers have moved on by the run and the entry of the sample behind the event is read again.  The loop's count
// of steps is a count of SAMPLES per scan (the prepared entries reach 63 samples ahead, a line has an end): {entry address of the
// call's first sample, samples left in the line} are at rctx + 32, a run that would take its scan beyond either is not served,
// and the count shrinks to what the scan that is furthest ahead still has -- in whole trips, counted from the copy the service was
// called from (BUDGET), and a scan that may not take the second step of the trip it was served in ends the loop as the count
// does (SHORT).  ENTER / LEAVE: the half trip that copy "a" owes lm and pp.  Whatever does not fit leaves the loop as before.
// (The C++ rendering of the loop in scan_group_decode.hip has the same service, statement by statement.)
// LD / ST / SZ: load / store of a sample, bytes per sample; ENEXT: the entry pair of the NEXT step; WHICH: from Ra in v108 and
// Rb in v109 to s[88:89] = the context of RItype 1; RECON: from the prediction in v112 and Errval (sign) in v114 to the sample
// in v112.
#define JLS_RUN_WHICH_LOSSLESS "v_cmp_eq_u32 s[88:89], v108, v109\n"
#define JLS_RUN_WHICH_NEAR                                                                                                         \
    "v_sad_u32 v91, v108, v109, v96\n"                                      /* |Ra - Rb| - NEAR */                               \
    "v_cmp_ge_i32 s[88:89], 0, v91\n"
#define JLS_RUN_RECON_LOSSLESS                                                                                                     \
    "v_add_u32 v112, v112, v114\n"                                                                                                \
    "v_and_b32 v112, %[smax], v112\n"
#define JLS_RUN_RECON_NEAR                                                                                                         \
    "v_mad_i32_i24 v112, v114, v94, v112\n"                                                                                       \
    "v_cmp_lt_i32 vcc, v112, v96\n"                                                                                               \
    "v_cmp_gt_i32 s[86:87], v112, v97\n"                                                                                          \
    "s_nop 1\n"                                                                                                                   \
    "v_cndmask_b32 v91, 0, v98, vcc\n"                                                                                            \
    "v_cndmask_b32_e64 v91, v91, v99, s[86:87]\n"                                                                                 \
    "v_add_u32 v112, v112, v91\n"                                                                                                 \
    "v_med3_i32 v112, v112, 0, %[smax]\n"
#define JLS_STEP_RARE(SFX, LD, ST, SZ, ENEXT, WHICH, RECON, ENTER, LEAVE, BUDGET, SHORT)                                                                      \
    "L_rare" SFX "%=:\n"                                                                                                          \
    "v_cndmask_b32_e64 v108, 0, 1, s[92:93]\n"                                                                                    \
    "v_and_b32 v109, 0xff, v123\n"                                                                                                \
    "v_cmp_eq_u32 s[94:95], %[where], %[recbase]\n"                         /* lanes in run mode */                              \
    "v_ashrrev_i32 %[ua], v108, %[ua]\n"                                                                                          \
    "v_ashrrev_i32 %[utb], v108, %[utb]\n"                                                                                        \
    "v_lshrrev_b32 v109, v108, v109\n"                                                                                            \
    "v_add_u32 %[un1], 1, v109\n"                                                                                                 \
    "s_or_b64 %[fail], s[96:97], s[94:95]\n"                                                                                      \
    "s_cbranch_scc0 L_back" SFX "%=\n"                                      /* nothing but the halving */                        \
    ENTER                                                                   /* lm and pp are true from here on */               \
    "s_cmp_lg_u64 s[96:97], 0\n"                                                                                                  \
    "s_cbranch_scc1 L_exit%=\n"                                             /* an unusual code somewhere: the loop ends anyway */ \
    /* -- every lane that stopped is in run mode */                                                                               \
    "s_mov_b64 s[90:91], exec\n"                                                                                                  \
    "s_mov_b64 exec, s[94:95]\n"                                                                                                  \
    "ds_read_b128 v[120:123], %[rctx]\n"                                    /* {RItype, A, N, Nn} of both run contexts */       \
    "ds_read_b128 v[124:127], %[rctx] offset:16\n"                                                                                \
    "ds_read_b64 v[116:117], %[rctx] offset:32\n"                           /* {entry of the call's first sample, samples left in its line} */ \
    LD " v108, %[lm]\n"                                                     /* Ra */                                             \
    /* the run-length code: `ones` complete blocks, a zero, J bits (src/scan_decoder_impl.hpp:280-298) */                        \
    "v_not_b32 v80, %[win]\n"                                                                                                     \
    "v_ffbl_b32 v80, v80\n"                                                 /* ones (0xFFFFFFFF: no zero in the window) */       \
    "v_add_u32 v81, %[ri], v80\n"                                           /* RUNindex behind the blocks */                     \
    "v_lshrrev_b32 v110, 2, v81\n"                                          /* J (RUNindex <= 16) */                             \
    "v_and_b32 v82, 3, v81\n"                                                                                                     \
    "v_add_u32 v82, 4, v82\n"                                                                                                     \
    "v_lshlrev_b32 v82, v110, v82\n"                                                                                              \
    "v_and_b32 v83, 3, %[ri]\n"                                                                                                   \
    "v_lshrrev_b32 v84, 2, %[ri]\n"                                                                                               \
    "v_add_u32 v83, 4, v83\n"                                                                                                     \
    "v_lshlrev_b32 v83, v84, v83\n"                                                                                               \
    "v_sub_u32 v82, v82, v83\n"                                             /* samples of the complete blocks */                 \
    "v_add_u32 v83, 1, v80\n"                                                                                                     \
    "v_lshrrev_b32 v84, v83, %[win]\n"                                      /* the bits behind the zero */                       \
    "v_bfrev_b32 v84, v84\n"                                                                                                      \
    "v_mov_b32 v85, 0\n"                                                                                                          \
    "v_cmp_ge_u32 s[82:83], 16, v80\n"                                      /* at most 16 blocks ... */                          \
    "v_cmp_ge_u32 s[84:85], 16, v81\n"                                      /* ... and RUNindex <= 16 behind them */             \
    "v_lshlrev_b64 v[84:85], v110, v[84:85]\n"                              /* v85 = the J bits */                               \
    "v_add_u32 v82, v82, v85\n"                                             /* run */                                            \
    "v_add_u32 v111, v83, v110\n"                                           /* bits of the run-length code */                    \
    "s_and_b64 s[84:85], s[84:85], s[82:83]\n"                                                                                    \
    "v_mad_u32_u24 v86, v82, " SZ ", %[lm]\n"                               /* slot of the last sample of the run */             \
    LD " v109, v86 offset:" SZ "\n"                                         /* Rb = the sample above the interruption sample */  \
    /* the run lies inside the line, inside the entries prepared for this call, and is at most G samples long */                 \
    "v_mbcnt_lo_u32_b32 v87, -1, 0\n"                                                                                             \
    "v_mbcnt_hi_u32_b32 v87, -1, v87\n"                                                                                           \
    "v_and_b32 v87, %[gl] - 1, v87\n"                                       /* this lane among the lanes of its scan */          \
    "v_cmp_ge_u32 s[82:83], %[gl], v82\n"                                                                                         \
    "s_and_b64 s[84:85], s[84:85], s[82:83]\n"                                                                                    \
    "s_waitcnt lgkmcnt(2)\n"                                                /* the call's first entry, samples left */           \
    "v_sub_u32 v88, %[pp], v116\n"                                                                                                \
    "v_lshrrev_b32 v88, 3, v88\n"                                           /* samples of this call before the event */          \
    "v_add_u32 v88, v88, v82\n"                                                                                                   \
    "v_add_u32 v88, 1, v88\n"                                               /* ... and with it */                                \
    "v_min_u32 v89, 63, v117\n"                                                                                                   \
    "v_cmp_le_u32 s[82:83], v88, v89\n"                                     /* (the interruption sample is one of the line's) */ \
    "v_sub_u32 v89, v89, v88\n"                                             /* samples the scan may still take in this call */   \
    "s_and_b64 s[84:85], s[84:85], s[82:83]\n"                                                                                    \
    /* behind it the code of the interruption sample */                                                                           \
    "v_lshrrev_b32 v113, v111, %[win]\n"                                                                                          \
    "v_ffbl_b32 v114, v113\n"                                               /* zeros of its prefix */                            \
    "v_add_u32 v115, 1, v114\n"                                                                                                   \
    "v_lshrrev_b32 v116, v115, v113\n"                                                                                            \
    "v_bfrev_b32 v116, v116\n"                                              /* the bits behind the prefix, first bit on top */   \
    "v_and_b32 v117, 0xff, %[cfg]\n"                                                                                              \
    "v_sub_u32 v117, v117, v110\n"                                          /* prefixes from here on are the escape */           \
    "v_bfe_u32 v90, %[cfg], 8, 8\n"                                         /* qbpp */                                           \
    "s_waitcnt lgkmcnt(0)\n"                                                                                                      \
    WHICH                                                                   /* s[88:89]: the context of RItype 1 */              \
    "v_cmp_lt_u32 s[86:87], v114, v117\n"                                   /* a regular code, not the escape */                 \
    "v_cmp_gt_u32 s[82:83], 32, v114\n"                                                                                           \
    "v_cndmask_b32_e64 v120, v120, v124, s[88:89]\n"                                                                              \
    "v_cndmask_b32_e64 v121, v121, v125, s[88:89]\n"                                                                              \
    "v_cndmask_b32_e64 v122, v122, v126, s[88:89]\n"                                                                              \
    "v_cndmask_b32_e64 v123, v123, v127, s[88:89]\n"                                                                              \
    "s_and_b64 s[84:85], s[84:85], s[82:83]\n"                                                                                    \
    /* k = min{k : N << k >= A + (N >> 1) RItype} (src/run_mode_context.hpp:34-62) */                                             \
    "v_lshrrev_b32 v124, 1, v122\n"                                                                                               \
    "v_mul_u32_u24 v124, v124, v120\n"                                                                                            \
    "v_add_u32 v124, v121, v124\n"                                                                                                \
    "v_max_u32 v125, 1, v124\n"                                                                                                   \
    "v_ffbh_u32 v125, v125\n"                                                                                                     \
    "v_ffbh_u32 v126, v122\n"                                                                                                     \
    "v_sub_u32 v125, v126, v125\n"                                                                                                \
    "v_max_i32 v125, 0, v125\n"                                                                                                   \
    "v_lshlrev_b32 v126, v125, v122\n"                                                                                            \
    "v_cmp_lt_u32 vcc, v126, v124\n"                                                                                              \
    "v_mov_b32 v112, v116\n"                                                                                                      \
    "v_mov_b32 v113, 0\n"                                                                                                         \
    "v_addc_co_u32 v125, vcc, 0, v125, vcc\n"                               /* k */                                              \
    "v_cndmask_b32_e64 v126, v90, v125, s[86:87]\n"                         /* bits behind the prefix: k, or qbpp (escape) */    \
    "v_add_u32 v127, v115, v126\n"                                                                                                \
    "v_add_u32 v111, v111, v127\n"                                          /* bits of the whole event */                        \
    "v_cmp_ge_u32 vcc, 24, v125\n"                                                                                                \
    "v_cmp_ge_u32 s[80:81], 32, v111\n"                                     /* all of it inside the window */                    \
    "v_lshlrev_b64 v[112:113], v126, v[112:113]\n"                          /* v113 = those bits */                              \
    "s_and_b64 s[84:85], s[84:85], vcc\n"                                                                                         \
    "s_and_b64 s[84:85], s[84:85], s[80:81]\n"                              /* the lanes served here */                          \
    "v_lshlrev_b32 v116, v125, v114\n"                                                                                            \
    "v_add_u32 v116, v116, v113\n"                                                                                                \
    "v_add_u32 v112, 1, v113\n"                                                                                                   \
    "v_cndmask_b32_e64 v116, v112, v116, s[86:87]\n"                        /* EMErrval */                                       \
    /* Errval (src/run_mode_context.hpp:86-99): |.| = (temp + map) >> 1 with temp = EMErrval + RItype, map = temp & 1; */         \
    /* negative iff (k != 0 or 2 Nn >= N) == map */                                                                               \
    "v_add_u32 v112, v116, v120\n"                                                                                                \
    "v_and_b32 v113, 1, v112\n"                                                                                                   \
    "v_add_u32 v112, v112, v113\n"                                                                                                \
    "v_lshrrev_b32 v112, 1, v112\n"                                                                                               \
    "v_lshlrev_b32 v114, 1, v123\n"                                                                                               \
    "v_cmp_ge_u32 vcc, v114, v122\n"                                                                                              \
    "v_min_u32 v114, 1, v125\n"                                                                                                   \
    "s_nop 0\n"                                                                                                                   \
    "v_cndmask_b32_e64 v114, v114, 1, vcc\n"                                                                                      \
    "v_xor_b32 v114, v114, v113\n"                                                                                                \
    "v_add_u32 v114, -1, v114\n"                                            /* -1 where Errval is negative */                    \
    "v_xor_b32 v112, v112, v114\n"                                                                                                \
    "v_sub_u32 v112, v112, v114\n"                                          /* Errval */                                         \
    /* the context (src/run_mode_context.hpp:65-83) */                                                                            \
    "v_lshrrev_b32 v113, 31, v112\n"                                                                                              \
    "v_add_u32 v123, v123, v113\n"                                                                                                \
    "v_sub_u32 v113, v116, v120\n"                                                                                                \
    "v_add_u32 v113, 1, v113\n"                                                                                                   \
    "v_lshrrev_b32 v113, 1, v113\n"                                                                                               \
    "v_add_u32 v121, v121, v113\n"                                                                                                \
    "v_xor_b32 v113, v122, v93\n"                                                                                                 \
    "v_sub_u32_e64 v113, 1, v113 clamp\n"                                   /* 1 where N = RESET */                              \
    "v_lshrrev_b32 v121, v113, v121\n"                                                                                            \
    "v_lshrrev_b32 v123, v113, v123\n"                                                                                            \
    "v_lshrrev_b32 v122, v113, v122\n"                                                                                            \
    "v_add_u32 v122, 1, v122\n"                                                                                                   \
    /* the sample: Ra + Errval where Ra and Rb are of one level, else Rb + Errval sign(Rb - Ra) (src/scan_decoder_core.hpp:72-100) */ \
    "v_sub_u32 v113, v109, v108\n"                                                                                                \
    "v_ashrrev_i32 v113, 31, v113\n"                                                                                              \
    "v_xor_b32 v114, v112, v113\n"                                                                                                \
    "v_sub_u32 v114, v114, v113\n"                                          /* Errval sign(Rb - Ra) */                           \
    "v_cndmask_b32_e64 v114, v114, v112, s[88:89]\n"                                                                              \
    "v_cndmask_b32_e64 v112, v109, v108, s[88:89]\n"                        /* the prediction: Rb, or Ra */                      \
    RECON                                                                                                                         \
    /* the lanes that were served */                                                                                              \
    "s_andn2_b64 s[94:95], s[94:95], s[84:85]\n"                            /* (the others stay stopped) */                      \
    "s_mov_b64 exec, s[84:85]\n"                                                                                                  \
    "s_cbranch_execz L_unserved" SFX "%=\n"                                                                                       \
    "v_cmp_lt_u32 vcc, v87, v82\n"                                          /* the lanes of the scan fill its run with Ra */     \
    "v_mad_u32_u24 v87, v87, " SZ ", %[lm]\n"                                                                                     \
    "v_cndmask_b32_e64 v113, 0, 16, s[88:89]\n"                                                                                   \
    "v_add_u32 v113, %[rctx], v113\n"                                                                                             \
    "ds_write_b128 v113, v[120:123]\n"                                                                                            \
    "s_and_b64 exec, exec, vcc\n"                                                                                                 \
    ST " v87, v108 offset:" SZ "\n"                                                                                               \
    "s_mov_b64 exec, s[84:85]\n"                                                                                                  \
    "v_mov_b32 %[lm], v86\n"                                                /* the next step stores the sample behind it */      \
    "v_lshl_add_u32 %[pp], v82, 3, %[pp]\n"                                                                                       \
    "ds_read_b64 " ENEXT ", %[pp] offset:8\n"                               /* the entry of the sample behind the event */       \
    "v_mov_b32 %[a], v112\n"                                                                                                      \
    "v_mov_b32 %[u1], v111\n"                                                                                                     \
    "v_mov_b32 %[k], 0\n"                                                                                                         \
    "v_mov_b32 v127, 0\n"                                                                                                         \
    "v_add_u32 %[where], 0xb68, %[recbase]\n"                               /* record 365 */                                     \
    "v_sub_u32_e64 %[ri], v81, 1 clamp\n"                                   /* RUNindex - 1, not below 0 */                      \
    /* the count of steps left: no more than any served scan may still take */                                                    \
    "s_mov_b64 s[82:83], exec\n"                                                                                                  \
    BUDGET                                                                                                                        \
    "L_budget" SFX "%=:\n"                                                                                                        \
    "s_ff1_i32_b64 s80, s[82:83]\n"                                                                                               \
    "s_nop 3\n"                                                            /* (a lane select written by the scalar unit) */     \
    "v_readlane_b32 s81, v89, s80\n"                                                                                              \
    "s_min_u32 %[cnt], %[cnt], s81\n"                                                                                             \
    "s_nop 0\n"                                                            /* (an SGPR written by the vector unit: 2 states) */ \
    "v_cmp_ne_u32 vcc, s81, v89\n"                                                                                                \
    "s_and_b64 s[82:83], s[82:83], vcc\n"                                                                                         \
    "s_cbranch_scc1 L_budget" SFX "%=\n"                                                                                          \
    "L_unserved" SFX "%=:\n"                                                                                                      \
    "s_waitcnt lgkmcnt(0)\n"                                                                                                      \
    "s_mov_b64 exec, s[90:91]\n"                                                                                                  \
    "s_mov_b64 %[fail], s[94:95]\n"                                                                                               \
    "s_cmp_lg_u64 s[94:95], 0\n"                                                                                                  \
    "s_cbranch_scc1 L_exit%=\n"                                                                                                   \
    SHORT                                                                   /* a served scan may not finish the trip */          \
    LEAVE                                                                                                                         \
    "s_branch L_back" SFX "%=\n"

#define JLS_STEP_EPILOGUE(EXIT_EXTRA, TRUE_UP_A)                                                                                   \
    "L_donea%=:\n"                                                          /* by count, out of copy "a" */                      \
    TRUE_UP_A                                                                                                                     \
    "L_doneb%=:\n"                                                                                                                 \
    "s_mov_b64 %[fail], 0\n"                                                                                                      \
    "L_exit%=:\n"                                                                                                                 \
    EXIT_EXTRA                                                                                                                    \
    "s_waitcnt lgkmcnt(0)\n"                                                /* (the compiler does not know of the last store) */ \
    "s_mov_b64 exec, s[98:99]\n"

// ORDER (three arguments): what is issued between the request of Q3 and its arrival, how many LDS operations may be outstanding
// when the ring words are awaited, and what is issued right behind the request of the record.  WINDOW_FIRST: commit + bit-window request, predictor, A.13 (the record's store right in front of the
// record request); UPDATE_FIRST: A.13 and the store first, so that the store has left the LDS queue when the record is requested.
#define JLS_STEP_ORDER_WINDOW_FIRST(PRED, RC, SZ, TOP_EXTRA, E0, E1) JLS_STEP_COMMIT_AND_WINDOW(SZ, TOP_EXTRA) PRED(RC, E0, E1) JLS_STEP_A13, "4", ""
// PREDICTOR_LATE: the predictor -- which nothing needs before the reconstruction -- behind the request of the record, where the
// wavefront would otherwise wait for it
#define JLS_STEP_ORDER_PREDICTOR_LATE(PRED, RC, SZ, TOP_EXTRA, E0, E1) JLS_STEP_COMMIT_AND_WINDOW(SZ, TOP_EXTRA) JLS_STEP_A13, "4", PRED(RC, E0, E1)
#define JLS_STEP_ORDER_UPDATE_FIRST(PRED, RC, SZ, TOP_EXTRA, E0, E1)                                                                    \
    JLS_STEP_A13 "ds_write2_b32 %[where], %[ua], v111 offset1:1\n" JLS_STEP_COMMIT_AND_WINDOW(SZ, TOP_EXTRA) PRED(RC, E0, E1), "3", ""
// (with UPDATE_FIRST the record's store is part of the order: the stores' macro then only has the sample)
#define JLS_STEP_STORES_SAMPLE_LATE(ST, OFF) "", "2", ST " %[lm], %[a]" OFF "\n", "1"
#define JLS_STEP_KSEEN "v_or_b32 %[kseen], %[kseen], %[k]\n"

// the loop: two steps per trip
#define JLS_STEP_BODY_X(...) JLS_STEP_BODY(__VA_ARGS__) // (ORDER(...) is three arguments once it is expanded)
// (copy "a" works on the entry in v[118:119] and requests the next one into v[106:107], copy "b" the other way round: the entry of a
// step stays valid to its end, so the predictor can sit behind the record request; the prologue loads the pair of copy "a", where
// every call starts)
#define JLS_STEP_LOOP_TEXT(RC, ASEL, PRED, SZ, LD, ORDER, ST, Q3_ADDR, Q3_OFFSET, TOP_EXTRA, K_EXTRA, A_EXTRA, EXIT_EXTRA, MODE, RARE_A, RARE_B)     \
    JLS_STEP_PROLOGUE                                                                                                              \
    JLS_STEP_BODY_X("a", JLS_STEP_TAIL_A, "v118", "v119", "v[106:107]", JLS_STEP_NEXT_ENTRY_A, RC, ASEL, SZ,                      \
                  ORDER(PRED, RC, SZ, JLS_STEP_ADVANCE_A(SZ) TOP_EXTRA, "v118", "v119"), JLS_STEP_STORES_LATE(ST, JLS_STEP_STORE_OFFSET_A(SZ)), \
                  Q3_ADDR, Q3_OFFSET, TOP_EXTRA, K_EXTRA, A_EXTRA, JLS_STEP_KSEEN, MODE)                                           \
    JLS_STEP_BODY_X("b", JLS_STEP_TAIL_B, "v106", "v107", "v[118:119]", "8", RC, ASEL, SZ,                                        \
                  ORDER(PRED, RC, SZ, JLS_STEP_ADVANCE_B(SZ) TOP_EXTRA, "v106", "v107"), JLS_STEP_STORES_LATE(ST, ""), Q3_ADDR,    \
                  Q3_OFFSET, TOP_EXTRA, K_EXTRA, A_EXTRA, JLS_STEP_KSEEN, MODE)                                                    \
    JLS_STEP_ENTER_B(SZ)                                                                                                           \
    RARE_A                                                                                                                         \
    RARE_B                                                                                                                         \
    JLS_STEP_EPILOGUE(EXIT_EXTRA, JLS_STEP_TRUE_UP_A(SZ))

#define JLS_STEP_LOOP_CLOBBERS                                                                                                     \
    "memory", "vcc", "scc", "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96",   \
        "s97", "s98", "s99", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107",      \
        "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124",  \
        "v125", "v126", "v127"

// the rare path of the four renderings (8-bit / wider samples, lossless / near-lossless), for the two copies of the step
#define JLS_STEP_RARE_A(LD, ST, SZ, WHICH, RECON)                                                                                 \
    JLS_STEP_RARE("a", LD, ST, SZ, "v[106:107]", WHICH, RECON, JLS_STEP_RARE_ENTER_A(SZ), JLS_STEP_RARE_LEAVE_A(SZ), JLS_STEP_BUDGET_A, JLS_STEP_SHORT_A)
#define JLS_STEP_RARE_B(LD, ST, SZ, WHICH, RECON) JLS_STEP_RARE("b", LD, ST, SZ, "v[118:119]", WHICH, RECON, "", "", JLS_STEP_BUDGET_B, "")
#define JLS_STEP_RARE_NARROW(SFX, WHICH, RECON) JLS_STEP_RARE_##SFX("ds_read_u8", "ds_write_b8", "1", WHICH, RECON)
#define JLS_STEP_RARE_WIDE(SFX, WHICH, RECON) JLS_STEP_RARE_##SFX("ds_read_u16", "ds_write_b16", "2", WHICH, RECON)
// cfg: escape_base | qbpp << 8 | RESET << 16 (escape_base: an event's escape prefix is escape_base - J); gl: lanes per scan
#define JLS_STEP_OPERANDS_OUT                                                                                                      \
    [a] "+v"(a), [p] "+v"(p), [lm] "+v"(lm), [pp] "+v"(pp), [where] "+v"(where), [ua] "+v"(u_a), [un1] "+v"(u_n1), [utb] "+v"(u_tb), \
        [cc] "+v"(u_cc), [u1] "+v"(u1), [k] "+v"(k_last), [kseen] "+v"(k_seen), [qsu] "+v"(qsu8), [win] "+v"(win_now),             \
        [cnt] "+s"(count), [fail] "=&s"(fail_m), [ri] "+v"(run_index)
#define JLS_STEP_OPERANDS_CHECKED , [mmseen] "+v"(mm_seen), [aseen] "+v"(a_seen_now), [tmm] "+v"(t_mm)
#define JLS_STEP_OPERANDS_IN                                                                                                       \
    [ring] "v"(ring_address), [recbase] "v"(records_address), [limitv] "v"(limit_v), [cfg] "v"(cfg_v), [inl] "s"(in_line_m),       \
        [smax] "s"(maxval_s), [rctx] "v"(run_ctx_address), [gl] "n"(G)

// 8-bit containers: how a step reads Ra, and its predictor (JLS_STEP_MED_FROM_RA)
#if JLS_STEP_MED_FROM_RA
#define JLS_STEP_NARROW_ASEL "BYTE_0"
#define JLS_STEP_NARROW_PRED JLS_STEP_PREDICTOR_FROM_RA
#else
#define JLS_STEP_NARROW_ASEL "DWORD"
#define JLS_STEP_NARROW_PRED JLS_STEP_PREDICTOR
#endif
#define JLS_STEP_LOOP_ASM_NARROW_MASKED()                                                                                          \
    asm volatile(JLS_STEP_LOOP_TEXT("BYTE_0", JLS_STEP_NARROW_ASEL, JLS_STEP_NARROW_PRED, "1", "ds_read_u8", JLS_STEP_ORDER_WINDOW_FIRST, \
                                    "ds_write_b8", "", " offset:255", "", "", "", "", JLS_STEP_LOSSLESS,      \
                                    JLS_STEP_RARE_NARROW(A, JLS_RUN_WHICH_LOSSLESS, JLS_RUN_RECON_LOSSLESS), JLS_STEP_RARE_NARROW(B, JLS_RUN_WHICH_LOSSLESS, JLS_RUN_RECON_LOSSLESS))                          \
                 : JLS_STEP_OPERANDS_OUT                                                                                           \
                 : JLS_STEP_OPERANDS_IN                                                                                            \
                 : JLS_STEP_LOOP_CLOBBERS)
#if JLS_STEP_MED_FROM_RA
// two texts in one kernel, chosen by the wave-uniform MAXVAL: 255 -- the sample stays unmasked inside the loop -- and the scans
// of 2 - 7 bits, which keep the mask
#define JLS_STEP_LOOP_ASM_NARROW()                                                                                                 \
    do                                                                                                                             \
    {                                                                                                                              \
        if (maxval_s == 255)                                                                                                       \
            asm volatile(JLS_STEP_LOOP_TEXT("BYTE_0", "BYTE_0", JLS_STEP_PREDICTOR_FROM_RA, "1", "ds_read_u8", JLS_STEP_ORDER_WINDOW_FIRST, \
                                            "ds_write_b8", "", " offset:255", "", "", "", JLS_STEP_EXIT_BYTE, \
                                            JLS_STEP_LOSSLESS_BYTE,                                                                \
                                            JLS_STEP_RARE_NARROW(A, JLS_RUN_WHICH_LOSSLESS, JLS_RUN_RECON_LOSSLESS), \
                                            JLS_STEP_RARE_NARROW(B, JLS_RUN_WHICH_LOSSLESS, JLS_RUN_RECON_LOSSLESS)) \
                         : JLS_STEP_OPERANDS_OUT                                                                                   \
                         : JLS_STEP_OPERANDS_IN                                                                                    \
                         : JLS_STEP_LOOP_CLOBBERS);                                                                                \
        else                                                                                                                       \
            JLS_STEP_LOOP_ASM_NARROW_MASKED();                                                                                     \
    } while (0)
#else
#define JLS_STEP_LOOP_ASM_NARROW() JLS_STEP_LOOP_ASM_NARROW_MASKED()
#endif

// wider samples: the difference is clamped to the table (-cap .. cap, cap = T3) and the table index needs its base added; the
// mapped error of a FINISHED step is accumulated (|Errval| > 65535 is invalid data), so is every updated A (2^24), and a
// code has to lie inside the 32-bit window (u + k < 32)
#define JLS_STEP_CHECKED_TOP "v_or_b32 %[mmseen], %[mmseen], v127\n"
#define JLS_STEP_CHECKED_K "v_add_u32 v112, v125, %[k]\n v_cmp_le_u32 vcc, 32, v112\n s_or_b64 s[96:97], s[96:97], vcc\n"
#define JLS_STEP_CHECKED_A "v_or_b32 %[aseen], %[aseen], %[ua]\n"
#define JLS_STEP_CHECKED_EXIT "v_mov_b32 %[tmm], v127\n"
#define JLS_STEP_WIDE_Q3 "v_med3_i32 v108, v108, v102, %[vcap]\n v_add_u32 v108, %[vcap], v108\n"
#define JLS_STEP_LOOP_ASM_WIDE()                                                                                                   \
    asm volatile("v_sub_u32 v102, 0, %[vcap]\n"                                                                                   \
                 JLS_STEP_LOOP_TEXT("WORD_0", "DWORD", JLS_STEP_PREDICTOR, "2", "ds_read_u16", JLS_STEP_ORDER_WINDOW_FIRST, "ds_write_b16", \
                                    JLS_STEP_WIDE_Q3, "", JLS_STEP_CHECKED_TOP, JLS_STEP_CHECKED_K, JLS_STEP_CHECKED_A,             \
                                    JLS_STEP_CHECKED_EXIT, JLS_STEP_LOSSLESS,                                                      \
                                    JLS_STEP_RARE_WIDE(A, JLS_RUN_WHICH_LOSSLESS, JLS_RUN_RECON_LOSSLESS), JLS_STEP_RARE_WIDE(B, JLS_RUN_WHICH_LOSSLESS, JLS_RUN_RECON_LOSSLESS))                            \
                 : JLS_STEP_OPERANDS_OUT JLS_STEP_OPERANDS_CHECKED                                                                 \
                 : JLS_STEP_OPERANDS_IN, [vcap] "v"(cap_v)                                                                         \
                 : JLS_STEP_LOOP_CLOBBERS)

// near-lossless scans, 8-bit and wider samples: the checks of the wide loop in both (a code may be longer than the window once
// qbpp is small; |Errval| and A are bounded by the same rules).  nr: NEAR | RANGE (2 NEAR + 1) << 8.
#define JLS_STEP_LOOP_ASM_NARROW_NEAR()                                                                                            \
    asm volatile(JLS_STEP_NEAR_CONSTANTS                                                                                           \
                 JLS_STEP_LOOP_TEXT("BYTE_0", JLS_STEP_NARROW_ASEL, JLS_STEP_NARROW_PRED, "1", "ds_read_u8", JLS_STEP_ORDER_WINDOW_FIRST, "ds_write_b8", \
                                    "", " offset:255", JLS_STEP_CHECKED_TOP, JLS_STEP_CHECKED_K, JLS_STEP_CHECKED_A,                \
                                    JLS_STEP_CHECKED_EXIT, JLS_STEP_NEAR, JLS_STEP_RARE_NARROW(A, JLS_RUN_WHICH_NEAR, JLS_RUN_RECON_NEAR), JLS_STEP_RARE_NARROW(B, JLS_RUN_WHICH_NEAR, JLS_RUN_RECON_NEAR)) \
                 : JLS_STEP_OPERANDS_OUT JLS_STEP_OPERANDS_CHECKED                                                                 \
                 : JLS_STEP_OPERANDS_IN, [nr] "s"(near_range_s)                                                                    \
                 : JLS_STEP_LOOP_CLOBBERS)
#define JLS_STEP_LOOP_ASM_WIDE_NEAR()                                                                                              \
    asm volatile("v_sub_u32 v102, 0, %[vcap]\n" JLS_STEP_NEAR_CONSTANTS                                                           \
                 JLS_STEP_LOOP_TEXT("WORD_0", "DWORD", JLS_STEP_PREDICTOR, "2", "ds_read_u16", JLS_STEP_ORDER_WINDOW_FIRST, "ds_write_b16", \
                                    JLS_STEP_WIDE_Q3, "", JLS_STEP_CHECKED_TOP, JLS_STEP_CHECKED_K, JLS_STEP_CHECKED_A,             \
                                    JLS_STEP_CHECKED_EXIT, JLS_STEP_NEAR, JLS_STEP_RARE_WIDE(A, JLS_RUN_WHICH_NEAR, JLS_RUN_RECON_NEAR), JLS_STEP_RARE_WIDE(B, JLS_RUN_WHICH_NEAR, JLS_RUN_RECON_NEAR)) \
                 : JLS_STEP_OPERANDS_OUT JLS_STEP_OPERANDS_CHECKED                                                                 \
                 : JLS_STEP_OPERANDS_IN, [vcap] "v"(cap_v), [nr] "s"(near_range_s)                                                 \
                 : JLS_STEP_LOOP_CLOBBERS)
