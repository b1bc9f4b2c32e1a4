"""Scan device assembly for out-of-line calls inside the kernels that carry SEVERAL chains per wavefront: the command line of
nuts_rs_amd/asm_scan.py's divergent-call rule (described there).  An `s_swappc_b64` inside a function whose name matches --kernels fails.

  python tools/check_divergent_calls.py file.s [--kernels REGEX]      (default: nuts_group_draw_kernel|nuts_lane)"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nuts_rs_amd"))
import asm_scan  # noqa: E402

path = sys.argv[1]
kernels = sys.argv[sys.argv.index("--kernels") + 1] if "--kernels" in sys.argv else asm_scan.SEVERAL_CHAINS
fs = asm_scan.divergent_calls(asm_scan.read(path), kernels)
for f in fs[:20]:
    print(f"{path}:{f.line}: {f.text}   (kernel {f.func})")
print(f"{path}: {len(fs)} out-of-line calls inside several-chains-per-wavefront kernels")
sys.exit(1 if fs else 0)
