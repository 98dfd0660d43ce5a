"""Wait states inside the decoder's inline assembly.  The assembler does not pad inline assembly, so a hazard the hardware
does not interlock (an SGPR written by the vector unit and read by the vector unit too soon) reads a stale value and nothing
reports it: a GPU test that happens to pass does not rule it out.  This compiles the decode kernels of
charls_amd/csrc/device/scan_group_decode.hip (the step loop of scan_group_step.inc among them) for gfx950 and checks every
;;#ASMSTART ... ;;#ASMEND region of the output against two rules:

  R1  an SGPR written by a VALU (v_readlane / v_readfirstlane destination, the SGPR or vcc destination of v_cmp*, a carry
      out) is read by a VALU -- as an operand or a lane mask -- only after at least 2 wait states;
  R2  an SGPR written by a VALU or a SALU is the lane select of v_readlane / v_writelane only after at least 4 wait states.

One instruction is one wait state, `s_nop N` is N + 1.  Paths are followed through straight-line code and through every
branch of the region to a label of the region (the budget loop of the rare path branches back to its top).

The rules are calibrated against hipcc (which pads what it emits itself): small kernels made of builtins must come out with
at least the wait states of the table.  For a SALU-written lane select hipcc pads fewer than 4; there R2 is the project's own
convention (the `s_nop 3` behind the step loop's s_ff1), kept because it costs nothing on the rare path.  CPU only."""
import os
import re
import shutil
import subprocess

import pytest

import common

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(common.ROOT, "charls_amd", "csrc")
pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="no hipcc")

R1_STATES = 2
R2_STATES = 4

# the kernels decode_launch.hip launches, one of each sample width x lossless / near-lossless x lines per row, and the fast decoder
INSTANTIATIONS = """
#include "device/scan_group_decode.hip"
#define JLS_GROUP(S, G, NL, W, K) template __global__ void jls::decode_scans_group<S, G, NL, W, K>(const jls::ScanDesc*, jls::ScanResult*, uint32_t);
JLS_GROUP(uint8_t, 16, 1, 1, false)
JLS_GROUP(uint16_t, 16, 1, 4, false)
JLS_GROUP(uint8_t, 8, 3, 1, false)
JLS_GROUP(uint8_t, 32, 1, 4, true)
JLS_GROUP(uint16_t, 8, 1, 1, true)
JLS_GROUP(uint16_t, 16, 4, 1, true)
template __global__ void jls::decode_scans_fast<uint8_t>(const jls::ScanDesc*, jls::ScanResult*);
template __global__ void jls::decode_scans_fast<uint16_t>(const jls::ScanDesc*, jls::ScanResult*);
"""

_CONTROL = ("s_nop", "s_waitcnt", "s_branch", "s_cbranch", "s_endpgm", "s_barrier", "s_sleep", "s_setprio", "s_trap", "s_sethalt",
            "s_icache", "s_dcache")


def _regs(text):
    """The 32-bit SGPR names an operand covers ('s[82:83]' -> s82 s83, 'vcc' -> vcc_lo vcc_hi); nothing for other operands."""
    text = text.strip()
    m = re.fullmatch(r"s(\d+)", text)
    if m:
        return {text}
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", text)
    if m:
        return {f"s{i}" for i in range(int(m.group(1)), int(m.group(2)) + 1)}
    for pair in ("vcc", "exec"):
        if text == pair:
            return {pair + "_lo", pair + "_hi"}
        if text in (pair + "_lo", pair + "_hi"):
            return {text}
    return set()


class Insn:
    def __init__(self, line):
        line = line.split(";")[0].split("//")[0].strip()
        self.text = line
        parts = line.split(None, 1)
        self.op = parts[0]
        # operands: up to the first modifier (clamp, offset:8, dst_sel:..., ...); a modifier has no comma in front of it
        self.operands = [o.strip().split()[0] for o in parts[1].split(",")] if len(parts) > 1 else []
        self.valu = self.op.startswith("v_")
        self.salu = self.op.startswith("s_") and not self.op.startswith(_CONTROL)
        self.states = int(self.operands[0], 0) + 1 if self.op == "s_nop" else 1
        self.lane_select = set()
        self.writes = set()
        self.reads = set()
        ops = self.operands
        if self.valu:
            dests = [0] if ops and _regs(ops[0]) else []
            if len(ops) > 1 and _regs(ops[1]) and ("_co_" in self.op or self.op.startswith(("v_mad_u64", "v_mad_i64", "v_div_scale"))):
                dests.append(1)  # the carry out
            self.writes = set().union(*(_regs(ops[i]) for i in dests)) if dests else set()
            sources = [o for i, o in enumerate(ops) if i not in dests]
            if self.op.startswith(("v_readlane", "v_writelane")) and len(ops) >= 3:
                self.lane_select = _regs(ops[2])
                sources = [o for i, o in enumerate(ops) if i not in dests and i != 2]
            self.reads = set().union(set(), *(_regs(o) for o in sources))
        elif self.salu and ops and not self.op.startswith(("s_cmp", "s_bitcmp")):
            self.writes = _regs(ops[0])
            if "saveexec" in self.op:
                self.writes |= {"exec_lo", "exec_hi"}
        self.target = ops[0] if self.op.startswith(("s_branch", "s_cbranch")) and ops else None


def regions(asm_text):
    """Every inline-assembly region of a .s file: a list of items, each ('label', name) or ('insn', Insn)."""
    out, cur = [], None
    for raw in asm_text.splitlines():
        s = raw.strip()
        if s.startswith(";;#ASMSTART"):
            cur = []
            continue
        if s.startswith(";;#ASMEND"):
            out.append(cur)
            cur = None
            continue
        if cur is None:
            continue
        s = s.split(";")[0].split("//")[0].strip()
        if not s or s.startswith("."):
            continue
        if s.endswith(":") and " " not in s:
            cur.append(("label", s[:-1]))
        else:
            cur.append(("insn", Insn(s)))
    return out


def _writers_before(region, pos, regs, need):
    """(writer, wait states between it and item `pos`) for every instruction that writes one of `regs` and reaches item `pos`
    within fewer than `need` wait states, on any path inside the region."""
    found = []
    branches = {}
    for i, (kind, x) in enumerate(region):
        if kind == "insn" and x.target is not None:
            branches.setdefault(x.target, []).append(i)
    stack = [(pos - 1, 0, False)]  # (the item looked at next, wait states so far, reached by a taken branch)
    seen = set()
    while stack:
        k, states, taken = stack.pop()
        if (k, states, taken) in seen:
            continue
        seen.add((k, states, taken))
        while k >= 0 and states < need:
            kind, x = region[k]
            if kind == "label":
                for b in branches.get(x, []):
                    stack.append((b, states, True))
            else:
                if x.op in ("s_branch", "s_endpgm", "s_setpc_b64") and not taken:
                    break  # nothing falls through an unconditional branch
                if x.writes & regs:
                    found.append((x, states))
                states += x.states
            taken = False
            k -= 1
    return found


def audit(asm_text):
    """Violations of R1 and R2 in the inline assembly of `asm_text`, and what was looked at."""
    violations = []
    stats = {"regions": 0, "valu_sgpr_writers": 0, "lane_selects": 0}
    for region in regions(asm_text):
        stats["regions"] += 1
        for pos, (kind, x) in enumerate(region):
            if kind != "insn":
                continue
            if x.valu and x.writes:
                stats["valu_sgpr_writers"] += 1
            if x.valu and x.reads:
                for w, states in _writers_before(region, pos, x.reads, R1_STATES):
                    if w.valu:
                        violations.append(f"R1: {w.text!r} -> {x.text!r}: {states} wait states, {R1_STATES} needed")
            if x.lane_select:
                stats["lane_selects"] += 1
                for w, states in _writers_before(region, pos, x.lane_select, R2_STATES):
                    if w.valu or w.salu:
                        violations.append(f"R2: {w.text!r} -> {x.text!r}: {states} wait states, {R2_STATES} needed")
    return sorted(set(violations)), stats


def _compile(tmp_path, source, name):
    src = tmp_path / (name + ".hip")
    src.write_text(source)
    out = tmp_path / (name + ".s")
    # the include flags of charls_amd/build.py (build() adds no defines of its own)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(common.ROOT, "include"), "-I" + CSRC,
                        "--cuda-device-only", "-S", "-x", "hip", str(src), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text()


def _kernel_body(asm_text, name):
    start = asm_text.index(name + ":")
    return asm_text[start:asm_text.index("s_endpgm", start)]


def _states_between(body, writer, reader):
    """Wait states hipcc put between the first instruction matching `writer` and the next one matching `reader`."""
    lines = [Insn(s.strip()) for s in body.splitlines() if s.strip() and not s.strip().startswith((".", ";")) and not s.strip().endswith(":")]
    w = next(i for i, x in enumerate(lines) if re.match(writer, x.text))
    r = next(i for i, x in enumerate(lines) if i > w and re.match(reader, x.text))
    return sum(x.states for x in lines[w + 1:r])


CALIBRATION = r"""
#include <hip/hip_runtime.h>
#include <stdint.h>
extern "C" __global__ void readlane_then_compare(const uint32_t* in, uint32_t* out, int lane)
{
    const uint32_t v = in[threadIdx.x];
    out[threadIdx.x] = v != __builtin_amdgcn_readlane(v, lane);
}
extern "C" __global__ void compare_then_select(const uint32_t* in, uint32_t* out)
{
    const uint32_t a = in[threadIdx.x], b = in[threadIdx.x + 64], c = in[threadIdx.x + 128], d = in[threadIdx.x + 192];
    out[threadIdx.x] = a > b ? c : d;
}
extern "C" __global__ void readlane_then_lane_select(const uint32_t* in, uint32_t* out)
{
    const uint32_t v = in[threadIdx.x];
    out[threadIdx.x] = __builtin_amdgcn_readlane(v, __builtin_amdgcn_readlane(v, 0) & 63u);
}
extern "C" __global__ void compare_then_lane_select(const uint32_t* in, uint32_t* out)
{
    const uint32_t v = in[threadIdx.x];
    out[threadIdx.x] = __builtin_amdgcn_readlane(v, (uint32_t)__ballot(v > 7u));
}
"""


def test_hipcc_pads_the_pairs_of_the_rule_table(tmp_path):
    asm = _compile(tmp_path, CALIBRATION, "calibration")
    # R1: a VALU-written SGPR as an operand, and as a lane mask
    assert _states_between(_kernel_body(asm, "readlane_then_compare"), r"v_readlane_b32 (s\d+)", r"v_cmp_") >= R1_STATES
    assert _states_between(_kernel_body(asm, "compare_then_select"), r"v_cmp_", r"v_cndmask_b32") >= R1_STATES
    # R2: a VALU-written lane select (a readlane's SGPR, a compare's vcc)
    assert _states_between(_kernel_body(asm, "readlane_then_lane_select"), r"v_readlane_b32 s\d+, v\d+, 0", r"v_readlane_b32 s\d+, v\d+, s") >= R2_STATES
    assert _states_between(_kernel_body(asm, "compare_then_lane_select"), r"v_cmp_", r"v_readlane_b32") >= R2_STATES


# the budget loop of the rare path as it stood with one wait state between v_readlane and the compare reading its SGPR
STALE_BUDGET_LOOP = """
;;#ASMSTART
s_mov_b64 s[82:83], exec
L_budget0:
s_ff1_i32_b64 s80, s[82:83]
s_nop 3
v_readlane_b32 s81, v89, s80
s_min_u32 s18, s18, s81
v_cmp_ne_u32 vcc, s81, v89
s_and_b64 s[82:83], s[82:83], vcc
s_cbranch_scc1 L_budget0
;;#ASMEND
"""


def test_the_audit_flags_known_violations():
    found, stats = audit(STALE_BUDGET_LOOP)
    assert found == ["R1: 'v_readlane_b32 s81, v89, s80' -> 'v_cmp_ne_u32 vcc, s81, v89': 1 wait states, 2 needed"]
    assert stats == {"regions": 1, "valu_sgpr_writers": 2, "lane_selects": 1}
    assert audit(STALE_BUDGET_LOOP.replace("s_min_u32 s18, s18, s81\n", "s_min_u32 s18, s18, s81\ns_nop 0\n"))[0] == []
    # a lane select written by the scalar unit too soon
    assert audit(STALE_BUDGET_LOOP.replace("s_min_u32 s18, s18, s81\n", "s_min_u32 s18, s18, s81\ns_nop 0\n")
                 .replace("s_nop 3\n", "s_nop 1\n"))[0] == [
        "R2: 's_ff1_i32_b64 s80, s[82:83]' -> 'v_readlane_b32 s81, v89, s80': 2 wait states, 4 needed"]
    # reached only through the branch back to the top of a loop: a mask written at the bottom, read at the top
    loop = """
;;#ASMSTART
L_top1:
v_cndmask_b32_e64 v1, v2, v3, s[4:5]
v_add_u32 v2, 1, v2
v_cmp_lt_u32 s[4:5], v2, v6
s_cbranch_scc1 L_top1
;;#ASMEND
"""
    assert audit(loop)[0] == ["R1: 'v_cmp_lt_u32 s[4:5], v2, v6' -> 'v_cndmask_b32_e64 v1, v2, v3, s[4:5]': 1 wait states, 2 needed"]
    assert audit(loop.replace("L_top1:\n", "L_top1:\ns_nop 0\n"))[0] == []
    # a carry out, and a VALU-written lane select; nothing is carried across an unconditional branch
    assert audit(";;#ASMSTART\nv_add_co_u32 v1, vcc, v2, v3\nv_addc_co_u32 v4, s[6:7], v5, v6, vcc\n;;#ASMEND\n")[0] == [
        "R1: 'v_add_co_u32 v1, vcc, v2, v3' -> 'v_addc_co_u32 v4, s[6:7], v5, v6, vcc': 0 wait states, 2 needed"]
    assert audit(";;#ASMSTART\nv_readfirstlane_b32 s9, v1\ns_nop 1\nv_writelane_b32 v2, s3, s9\n;;#ASMEND\n")[0] == [
        "R2: 'v_readfirstlane_b32 s9, v1' -> 'v_writelane_b32 v2, s3, s9': 2 wait states, 4 needed"]
    assert audit(";;#ASMSTART\nv_cmp_eq_u32 vcc, v1, v2\ns_branch L_x2\nL_y2:\nv_cndmask_b32_e32 v3, v4, v5, vcc\nL_x2:\n;;#ASMEND\n")[0] == []


def test_the_decode_kernels_keep_their_wait_states(tmp_path):
    asm = _compile(tmp_path, INSTANTIATIONS, "decode_kernels")
    found, stats = audit(asm)
    # what the audit must have seen: the step loops of six group kernels (with their rare paths) and the fast decoder's asm
    assert stats["regions"] >= 150, stats
    assert stats["valu_sgpr_writers"] >= 6 * 20, stats
    assert stats["lane_selects"] >= 6 * 2, stats
    assert "L_budget" in asm
    assert found == [], "\n".join(found)
