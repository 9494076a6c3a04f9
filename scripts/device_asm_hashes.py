"""sha256 of the device-only assembly of every .hip source of a tree, for comparing two trees' device code.

  python scripts/device_asm_hashes.py [tree root] > hashes.json

The project's own flags plus --cuda-device-only -S.  Lines that carry a path, the compilation unit's id (__hip_cuid_*, a hash
of the path) or the compiler's ident are dropped before hashing, so two checkouts at different places compare equal when their
device code is the same; keeping both at the same path depth leaves little to drop.
"""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def main():
    root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
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
        return src, {"sha256": hashlib.sha256("".join(kept).encode()).hexdigest(), "lines": len(kept)}

    with ThreadPoolExecutor(max_workers=4) as pool:
        print(json.dumps(dict(pool.map(one, sources)), indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
