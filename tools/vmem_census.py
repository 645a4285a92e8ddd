"""Static census of the step kernels' vector-memory reads (needs hipcc, no GPU).

  python tools/vmem_census.py [-o FILE]

Compiles the four instantiations of mre_kernels.hip to gfx950 assembly with the flags of lib.build() and prints, for
every phase function and kernel: the vector-memory loads (global_load_* / flat_load_*), the GROUPS they fall into --
a group is a run of loads with no full drain (`s_waitcnt vmcnt(0)`) between them, i.e. one round trip to memory that
the wave waits for on its own --, the instructions, the VGPRs, the scratch bytes and, for kernels, the SGPR / VGPR
spill counts and the occupancy the compiler reports.  It is ONE linear pass through each function's text: loops and
exec-masked branches make the dynamic numbers differ.  Use it to compare two builds of the same source, not as a
measurement.
"""
import argparse, os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mujoco_robot_environments_amd import lib
CSRC = os.path.join(ROOT, "mujoco_robot_environments_amd", "csrc")
# the step kernel's instantiations as lib.build() compiles them, in the order of its table
UNITS = [(f"{name} ({what})", defines) for (name, src, defines), what in
         zip([u for u in lib.UNITS if u[1] == lib.STEP_SOURCE], ("compact PGS", "large PGS", "compact Newton", "large Newton"))]
# the phases one step of the flagship (Newton) workload runs outside the solver, in the order of the step
STEP_PHASES = ["position_stage", "gripper_local", "connect_rows_local", "velocity_stage", "finger_bias", "collide_broad",
               "collide_narrow",
               "assemble_constraints", "arm_actuation", "smooth_forces_assemble", "integrate_setup", "integrate"]

LOAD = re.compile(r"^\s+(global_load|flat_load)_")
INSTR = re.compile(r"^\s+[a-z]\w+")
DRAIN = re.compile(r"^\s+s_waitcnt\b.*\bvmcnt\(0\)")
LABEL = re.compile(r"^(_Z\w+):")


def short(mangled):
    m = re.match(r"_ZN3mre(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    return mangled[len(m.group(0)):len(m.group(0)) + n]


def census(asm):
    """-> list of (name, dict) in file order"""
    out, cur, meta = [], None, {}
    for line in asm.splitlines():
        m = LABEL.match(line)
        if m:
            cur = dict(name=short(m.group(1)), loads=0, groups=0, open=False, instr=0, vgpr=None, scratch=None, occ=None)
            out.append(cur)
            continue
        m = re.match(r"\s+\.name:\s+(_Z\w+)", line)
        if m:
            meta_cur = meta.setdefault(short(m.group(1)), {})
            continue
        m = re.match(r"\s+\.(sgpr_spill_count|vgpr_spill_count):\s+(\d+)", line)
        if m and meta:
            meta_cur[m.group(1)] = int(m.group(2))
            continue
        if cur is None:
            continue
        if line.startswith("; NumVgprs:"):
            cur["vgpr"] = int(line.split(":")[1])
        elif line.startswith("; ScratchSize:"):
            cur["scratch"] = int(line.split(":")[1])
        elif line.startswith("; Occupancy:"):
            cur["occ"] = int(line.split(":")[1])
        elif line.startswith(".Lfunc_end"):
            if cur["open"]:
                cur["groups"] += 1
                cur["open"] = False
        elif LOAD.match(line):
            cur["loads"] += 1
            cur["instr"] += 1
            cur["open"] = True
        elif DRAIN.match(line):
            cur["instr"] += 1
            if cur["open"]:
                cur["groups"] += 1
                cur["open"] = False
        elif INSTR.match(line) and not line.lstrip().startswith("."):
            cur["instr"] += 1
    for f in out:
        f.update(meta.get(f["name"], {}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lines = ["# vector-memory census of the step units (tools/vmem_census.py): static, one pass through each function",
             "# loads = global_load_* + flat_load_*; groups = runs of loads ended by s_waitcnt vmcnt(0)"]
    with tempfile.TemporaryDirectory() as td:
        procs = []
        for k, (name, flags) in enumerate(UNITS):
            s = os.path.join(td, f"u{k}.s")
            procs.append((name, s, subprocess.Popen([hipcc] + lib.FLAGS + flags + ["--cuda-device-only", "-S",
                                                    os.path.join(CSRC, lib.STEP_SOURCE), "-o", s],
                                                    stderr=subprocess.DEVNULL)))
        for name, s, p in procs:
            if p.wait() != 0:
                sys.exit(f"hipcc failed on {name}")
            with open(s) as fh:
                fs = census(fh.read())
            lines.append("")
            lines.append(f"== {name}")
            lines.append(f"{'function':34s} {'loads':>6s} {'groups':>7s} {'instr':>7s} {'vgpr':>5s} {'scratch':>8s} "
                         f"{'sgpr_spill':>11s} {'vgpr_spill':>11s} {'occupancy':>10s}")
            for f in fs:
                kern = "sgpr_spill_count" in f
                lines.append(f"{f['name']:34s} {f['loads']:6d} {f['groups']:7d} {f['instr']:7d} {f['vgpr']:5d} "
                             f"{f['scratch']:8d} {(str(f['sgpr_spill_count']) if kern else '-'):>11s} "
                             f"{(str(f['vgpr_spill_count']) if kern else '-'):>11s} "
                             f"{(str(f['occ']) if f['occ'] is not None else '-'):>10s}")
            by = {f["name"]: f for f in fs}
            ph = [by[n] for n in STEP_PHASES if n in by]
            lines.append(f"{'per-step phases, sum':34s} {sum(f['loads'] for f in ph):6d} {sum(f['groups'] for f in ph):7d}")
    text = "\n".join(lines) + "\n"
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
