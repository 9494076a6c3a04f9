"""sha256 of the device-only assembly of every .hip source of a tree, for comparing two trees' device code.

  python scripts/device_asm_hashes.py [tree root] > hashes.json                  one hash per unit
  python scripts/device_asm_hashes.py --per-kernel [tree root] > hashes.json     one hash per kernel, over the whole tree

The project's own flags plus --cuda-device-only -S.  Lines that carry a path, the compilation unit's id (__hip_cuid_*, a hash
of the path) or the compiler's ident are dropped before hashing, so two checkouts at different places compare equal when their
device code is the same; keeping both at the same path depth leaves little to drop.

--per-kernel is for a change that moves kernels between units: it cuts every unit's assembly at the functions' symbols (from a
"-- Begin function" line to the end of the resource comments after "-- End function") and prints {symbol: sha256} for all
of them.  hipcc numbers a function's local labels by the function's position in its unit (.LBB<k>_<n>, .Lfunc_end<k>, BB<k>_<n>
in comments) and pads the comments after a label to a column; the index is taken out and runs of blanks become one, so a
kernel compares equal wherever it stands.  A symbol that two units define is an error.
"""
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

BEGIN = re.compile(r"; -- Begin function (\S+)")
POSITION = re.compile(r"(?<![A-Za-z0-9_])(\.LBB|BB|\.Lfunc_begin|\.Lfunc_end)\d+")


def per_kernel(lines):
    """{symbol: sha256} of the functions in one unit's (already filtered) assembly."""
    out, name, chunk, ended = {}, None, [], False
    for l in lines + ["\t.section\t.text.\n"]:
        if name and ended and l.startswith(("\t.section\t.text", "\t.text", "\t.section\t.AMDGPU.gpr_maximums")):
            out[name] = hashlib.sha256("".join(chunk).encode()).hexdigest()
            name = None
        m = BEGIN.search(l)
        if m:
            name, chunk, ended = m.group(1), [], False
        if name:
            chunk.append(re.sub(r"[ \t]+", " ", POSITION.sub(r"\1", l)))
            ended = ended or "-- End function" in l
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--per-kernel"]
    kernels = len(args) != len(sys.argv) - 1
    root = os.path.abspath(args[0] if args else os.path.join(os.path.dirname(__file__), ".."))
    spec = importlib.util.spec_from_file_location("_build", os.path.join(root, "constraint_solver_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    sources = [s for s in b.HIP_SOURCES if s.endswith(".hip")]

    def one(src):
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, src + ".s")
            b._run([b._hipcc()] + b.HIP_FLAGS + ["--cuda-device-only", "-S", os.path.join(b.CSRC, src), "-o", out])
            with open(out) as f:
                kept = [l for l in f if root not in l and "/" + src not in l and ".ident" not in l and ".file" not in l and "__hip_cuid_" not in l]
        if kernels:
            return src, per_kernel(kept)
        return src, {"sha256": hashlib.sha256("".join(kept).encode()).hexdigest(), "lines": len(kept)}

    with ThreadPoolExecutor(max_workers=4) as pool:
        units = dict(pool.map(one, sources))
    if kernels:
        merged = {}
        for src, found in units.items():
            for name, h in found.items():
                if name in merged:
                    raise SystemExit("%s is defined by two units (the second: %s)" % (name, src))
                merged[name] = h
        units = merged
    print(json.dumps(units, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
