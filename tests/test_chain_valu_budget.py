"""Vector-instruction budget of the row-chained kernel's benchmark instantiation (csrc/chain_device.h), no GPU needed (hipcc
cross-compiles gfx950 to assembly).

fp32 MFMAs and vector-ALU instructions exclude each other on a SIMD (profiles/r06_mfma_valu_lab.log: 2 / 4 / 8 v_fma per 8 MFMAs
cost 9 / 14 / 21 % of the MFMA rate, from either wave of the SIMD), so the vector instructions a pass carries beside its 4,736 MFMAs
are the distance to the peak.  Three kinds were there for no reason and must not come back:
* scalars parked in lanes of a VGPR (hipcc's answer to a full scalar register file) and fetched with v_readlane_b32 inside the step
  loops;
* ReLU as two v_max_f32 per value (a canonicalising v_max x, x in front of the v_max against the floor);
* per-step rebuilds of lane constants, bias transposes through register moves — counted through the phase totals.
The kernel marks its phases with comment lines (`; dctr_chain phase: main / tail / end`): everything between two of them is
counted for the first, the once-per-launch parameter loads in front of `main` for neither.  Counted that way the parent of this
test's commit had 2353 (main) and 2042 (tail) vector instructions; the bounds below are the smaller counts its pass loops alone had."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TU = "chain_kernels_r2w8_m42.hip"
KERNEL = "ILi2ELi8ELi1ELb0ELi4ELi2ELi1ELb1E"      # chain_kernel<2, 8, 1, false, 4, 2, 1, true, ...>: bench.py's DeepFM forward

# static counts of the parent commit's pass loops: (vector instructions, v_max_f32) per phase — the new counts must be strictly below
PARENT = {"main": (1659, 385), "tail": (1515, 225)}
# what this commit reached: the baseline of the next change, not a bound
ACHIEVED = {"main": (1214, 224), "tail": (889, 112)}

_NO_DST = ("ds_write", "global_store", "global_load_lds", "buffer_store", "flat_store", "scratch_store", "global_atomic")


@pytest.fixture(scope="module")
def phases(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("valu") / (TU + ".s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "deepctr_amd", "csrc"), "-x", "hip", "--cuda-device-only", "-S",
           os.path.join(ROOT, "deepctr_amd", "csrc", TU), "-o", str(out)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert proc.returncode == 0, proc.stdout[-2000:]
    lines = open(str(out)).read().split("\n")
    start = [i for i, l in enumerate(lines) if re.match(r"^_ZN10dctr_chain12chain_kernel" + KERNEL + r"\w*:", l)]
    assert len(start) == 1, "instantiation %s: %d definitions" % (KERNEL, len(start))
    end = next(i for i in range(start[0], len(lines)) if "s_endpgm" in lines[i])
    # basic blocks: cut at labels and behind branches; the phase of a block is that of the last marker in front of it
    blocks, phase = {"main": [], "tail": []}, None
    cur = []

    def close():
        if cur and phase in blocks:
            blocks[phase].append(list(cur))
        del cur[:]

    for l in lines[start[0] + 1:end + 1]:
        m = re.search(r"dctr_chain phase: (\w+)", l)
        if m:
            close()
            phase = m.group(1)
            continue
        s = l.split(";")[0].strip()
        if not s or s.startswith("."):
            if re.match(r"^\.LBB\w+:", s):
                close()
            continue
        if re.match(r"^\w+:", s):
            close()
            continue
        cur.append(s)
        if s.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            close()
    close()
    assert phase == "end" and blocks["main"] and blocks["tail"], "phase markers missing from the assembly"
    return blocks


def _is_valu(s):
    return s.startswith("v_") and not s.startswith("v_mfma")


def _regs(op):
    """VGPR numbers an operand names (v7, v[4:7]); nothing for scalars and constants."""
    m = re.match(r"^v(\d+)$", op)
    if m:
        return {int(m.group(1))}
    m = re.match(r"^v\[(\d+):(\d+)\]$", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def _operands(s):
    parts = s.split(None, 1)
    return [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []


def test_no_lane_parked_scalars_beside_the_mfmas(phases):
    for name, blocks in phases.items():
        for b in blocks:
            mfma = sum(1 for s in b if s.startswith("v_mfma"))
            lane = [s for s in b if s.startswith(("v_readlane_b32", "v_writelane_b32"))]
            assert not (mfma >= 16 and lane), "%s phase: a block of %d MFMAs holds %s" % (name, mfma, lane[:4])


def test_one_v_max_per_activated_value(phases):
    for name, blocks in phases.items():
        for b in blocks:
            fresh = set()                              # registers last written by a v_max_f32 of this block
            for s in b:
                ops = _operands(s)
                if s.startswith("v_max_f32"):
                    assert len(ops) == 3, s
                    assert ops[1] != ops[2], "%s phase: canonicalising %s" % (name, s)
                    src = _regs(ops[1]) | _regs(ops[2])
                    assert not (src & fresh), "%s phase: %s takes the result of another v_max_f32" % (name, s)
                    fresh |= _regs(ops[0])
                elif ops and not s.startswith(_NO_DST):
                    fresh -= _regs(ops[0])


def test_static_vector_instructions_below_the_parent(phases):
    got = {}
    for name, blocks in phases.items():
        valu = sum(1 for b in blocks for s in b if _is_valu(s))
        vmax = sum(1 for b in blocks for s in b if s.startswith("v_max_f32"))
        mfma = sum(1 for b in blocks for s in b if s.startswith("v_mfma"))
        got[name] = (valu, vmax, mfma)
    msg = "static (VALU, v_max_f32, MFMA) per phase: %r; parent (VALU, v_max_f32): %r; reached by the commit that added this test: %r" % (
        got, PARENT, ACHIEVED)
    print(msg)
    for name in ("main", "tail"):
        assert got[name][0] < PARENT[name][0] and got[name][1] < PARENT[name][1], msg
