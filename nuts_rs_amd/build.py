"""Build libnuts_amd.so (the HIP engine) in-tree for gfx950.  `python -m nuts_rs_amd.build [--force] [-v]`.

The kernels of each density live in their own translation unit (csrc/kern_*.hip) so the build runs in parallel;
every unit is compiled with hipcc --offload-arch=gfx950 (cross-compiles without a GPU) and the objects are linked
into one shared library that exports the C ABI of include/nuts_amd.h.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
LIB = os.path.join(HERE, "libnuts_amd.so")
# (the slowest translation units first: the build is as long as its longest chain of jobs on the available cores)
UNITS = ["kern_tile_mvn_prec.hip", "kern_tile_mvn_diag.hip", "kern_lockstep.hip", "kern_lr_mvn_prec.hip@large", "kern_lr_mvn_prec.hip@small",
         "kern_kin_mvn_prec.hip@large", "kern_kin_mvn_prec.hip@small", "kern_mvn_prec.hip@large", "kern_mvn_prec.hip@small", "kern_lr_iid_normal.hip@large",
         "kern_lr_iid_normal.hip@small", "kern_lr_diag_normal.hip@large", "kern_lr_diag_normal.hip@small", "kern_lr_funnel.hip@large", "kern_lr_funnel.hip@small",
         "kern_lr_host_cb.hip@large", "kern_lr_host_cb.hip@small", "kern_kin_iid_normal.hip@large", "kern_kin_iid_normal.hip@small", "kern_kin_diag_normal.hip@large",
         "kern_kin_diag_normal.hip@small", "kern_kin_funnel.hip@large", "kern_kin_funnel.hip@small", "kern_kin_host_cb.hip@large", "kern_kin_host_cb.hip@small", "kern_lane.hip",
         "kern_lane_kin.hip", "kern_iid_normal.hip@large", "kern_iid_normal.hip@small", "kern_diag_normal.hip@large", "kern_diag_normal.hip@small", "kern_funnel.hip@large",
         "kern_funnel.hip@small", "kern_host_cb.hip@large", "kern_host_cb.hip@small", "unit_batch.hip", "nuts_engine.hip", "kern_cluster.hip", "kern_cluster_kin.hip", "kern_eight_schools.hip@inl",
         "kern_lr_eight_schools.hip@inl", "kern_kin_eight_schools.hip@inl", "math_seam.hip", "probe_bw.hip", "pooled_reduce.hip", "pooled_scatter.hip", "lowrank_device.hip", "kern_expand.hip@inl", "summary.hip", "quantile.hip", "rank_transform.hip@inl", "stats_diag.hip", "lowrank_host.cpp"]
# (lowrank_host.cpp holds both ISA builds of the host estimator in ONE translation unit: per-function target attributes, see there)
# Variants of a unit ("file@variant": its own object, the flags below).  A density's one-chain kernels are TWO units from one source
# (nuts_launch.hpp NM_TU_PART): "small" = the tilings of <= 4 doubles per lane + the small-chain kernels with EVERY special function inlined — no
# out-of-line device call (fourth incident; the scan below rejects an s_swappc_b64 there) —, "large" = the 8- and 16-doubles tilings with
# the calls (inlined they cost K2 11 %); "inl" = a unit that only has small tilings (8 schools), or whose lanes work on different rows
# (kern_expand.hip, the expansion pass: nuts_expand.hpp; rank_transform.hip, whose score kernel evaluates dlog per element).
VARIANT_FLAGS = {"": [], "small": ["-DNM_TU_PART=1", "-DNM_DETMATH_INLINE=1"], "large": ["-DNM_TU_PART=2"], "inl": ["-DNM_DETMATH_INLINE=1"]}
NO_CALL_VARIANTS = ("small", "inl")
# -ffp-contract=off: FMAs only where the reference writes mul_add
# -Wno-pass-failed: "loop not unrolled" remarks of the matrix-core kernel's partially unrolled product loops (a diagnostic only)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-pass-failed"]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _includes(path, seen=None):
    """The quoted includes a source pulls in (recursively, resolved against csrc/ and include/): a unit is recompiled when
    one of ITS headers changed, not when any header did (nuts_tile.hpp concerns two units of 26)."""
    import re
    seen = set() if seen is None else seen
    try:
        text = open(path).read()
    except OSError:
        return seen
    for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, flags=re.M):
        for base in (os.path.dirname(path), CSRC, os.path.join(HERE, "..", "include")):
            q = os.path.normpath(os.path.join(base, name))
            if os.path.exists(q):
                if q not in seen:
                    seen.add(q)
                    _includes(q, seen)
                break
    return seen


def _src(u):
    return os.path.join(CSRC, u.split("@")[0])


def _obj(u):
    name, _, variant = u.partition("@")
    return os.path.join(OBJ, name.replace(".hip", "").replace(".cpp", "") + ("_" + variant if variant else "") + ".o")


def _unit_stale(u):
    src = _src(u)
    return _newer(_obj(u), [src] + sorted(_includes(src)))


def needs_build():
    """True when the library is missing, older than one of its objects, or an object is older than its source / its headers."""
    return any(_unit_stale(u) for u in UNITS) or _newer(LIB, [_obj(u) for u in UNITS])


class StoreHazardError(RuntimeError):
    """A finding of any rule of nuts_rs_amd/asm_scan.py but the exec-spill one: a buffer store whose data registers are rewritten inside the hazard
    window, a call where the build allows none, a VALU hazard without its wait states."""


class ExecSpillError(RuntimeError):
    """The compiler placed a VGPR spill / reload before the exec restore of a join block that is entered with EXEC == 0 (the root
    cause of the code-generation incidents of rounds 4 - 5) and the instance could not be repaired in the assembly."""


# what to tell the author of the code, by rule (asm_scan.py's ids; valu-A .. valu-G share a line)
ADVICE = {
    "exec-spill": "join block(s) with VGPR spill code before the exec restore (DESIGN §22; where not [fixable] in the assembly: perturb the source or "
                  "build the unit with -mllvm -amdgpu-spill-sgpr-to-vgpr=false)",
    "store-hazard": "unguarded store-data hazard(s) in the generated assembly (guard the store as buf_store2 / LCtx::bst do, DESIGN §15)",
    "store-hazard-mubuf64": "unguarded store-data hazard(s), 64-bit MUBUF stores included (guard the store as buf_store2 / LCtx::bst do, DESIGN §15)",
    "divergent-call": "out-of-line call(s) inside a several-chains-per-wavefront kernel (force-inline the callee, DESIGN §22)",
    "valu": "software-managed VALU hazard(s) without their wait states (DESIGN §22)",
    "device-call": "out-of-line device call(s) (s_swappc_b64) in a unit that is built without them (-DNM_DETMATH_INLINE=1; DESIGN §22): mark the callee(s) "
                   "__forceinline__ (a __noinline__ helper in a user density of a small tiling is not supported)"}


def _report(what, findings):
    """The finding records as a message: per rule its advice and the first twenty records."""
    out = []
    for rule in dict.fromkeys(f["rule"] for f in findings):
        fs = [f for f in findings if f["rule"] == rule]
        out.append(f"{what}: {len(fs)} {ADVICE[rule[:4] if rule.startswith('valu-') else rule]}:")
        out += [f"    {f['func']}: line {f['line']}: {f['text']}" + (f"   <- line {f['prod_line']}: {f['prod_text']}" if f["prod_line"] else "")
                + (f"   (block {f['detail']['block']}{', [fixable]' * f['detail']['fixable']})" if f["detail"] else "") for f in fs[:20]]
    return "\n".join(out)


def _asm_scan(asm_path, allow_calls, fix=None):
    """asm_scan.py on one device assembly -> its finding records.  ONE child interpreter, started by file path (it imports the standard library
    only); a child, because the units are compiled from a thread pool and in-process scans of seconds each would queue on the interpreter lock.
    The scanner is part of the package: no build goes without it, and a child that does not answer with records is an error."""
    import json
    args = [sys.executable, os.path.join(HERE, "asm_scan.py"), asm_path] + ([] if allow_calls else ["--no-calls"]) + (["--fix", fix] if fix else [])
    r = subprocess.run(args, capture_output=True, text=True)
    records = [json.loads(l) for l in r.stdout.splitlines()] if r.returncode in (0, 1) else []
    if r.returncode != 0 and not records:
        raise RuntimeError(f"the assembly scan did not run ({' '.join(args)}):\n" + r.stderr[-3000:])
    return records


def _replay(cmd, what):
    """Re-run hipcc's own pipeline from the device assembler on (the commands `hipcc -###` shows for the same arguments): assembler, lld,
    bundler, host compile.  For ONE offload architecture: with a second one the replay would assemble that one's unrepaired file as well."""
    import shlex
    plan = subprocess.run(cmd + ["-###"], capture_output=True, text=True).stderr.split("\n")
    steps = [shlex.split(l) for l in plan if l.lstrip().startswith('"')]
    device_as = [k for k, c in enumerate(steps) if "-cc1as" in c and "amdgcn-amd-amdhsa" in c]
    if len(device_as) != 1:
        raise ExecSpillError(f"{what}: cannot replay the compiler pipeline on the repaired assembly: `hipcc -###` shows {len(device_as)} device assembler "
                             "steps, and the replay is written for exactly one (a single --offload-arch)")
    for c in steps[device_as[0]:]:
        if not ("-E" in c and "-cc1" in c):          # (the host preprocessor step: its output is unchanged)
            subprocess.check_call(c)


def _scan_unit(asm_path, cmd, what, allow_calls=True):
    """Every rule on one device assembly; a finding fails the build.  All but this: an exec-spill finding (a miscompile of ROCm 7.2's hipcc, DESIGN
    §22) that asm_scan.py can prove movable is repaired where the defect is — the exec restore moves up to the block's first instruction in the
    ASSEMBLY, the rest of hipcc's pipeline is replayed on the repaired file, and that file is scanned again."""
    findings = _asm_scan(asm_path, allow_calls, fix=asm_path + ".fixed")
    repaired = bool(findings) and all(f["detail"] and f["detail"]["fixable"] for f in findings)
    if repaired:
        print("nuts_rs_amd.build: repaired in the assembly:\n" + _report(what, findings), file=sys.stderr)
        os.replace(asm_path + ".fixed", asm_path)
        _replay(cmd, what)
        findings = _asm_scan(asm_path, allow_calls)
    if findings:          # (the message names all of them: a fixable spill beside another rule's finding is repaired once that one is gone)
        stuck = any(f["detail"] and (repaired or not f["detail"]["fixable"]) for f in findings)
        raise (ExecSpillError if stuck else StoreHazardError)(_report(what, findings))


def _compile_scanned(hipcc, flags, src, out, what, link=False, allow_calls=True):
    """Compile `src` (one hipcc run: -save-temps keeps the device assembly the object is assembled from), scan it, drop the temporaries."""
    import shutil
    import tempfile
    tmp = tempfile.mkdtemp(prefix="nm_tmp_", dir=os.path.dirname(out) or ".")
    try:
        # (-save-temps=obj writes next to the OUTPUT: compile into the temporary directory, then move the product out)
        prod = os.path.join(tmp, os.path.basename(out))
        cmd = [hipcc] + flags + ["-save-temps=obj"] + ([] if link else ["-c"]) + [src, "-o", prod]
        subprocess.check_call(cmd)
        asms = [os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith(".s") and "amdgcn" in f]
        if not asms and not src.endswith(".cpp"):
            raise RuntimeError(f"{what}: no device assembly among the compiler's temporaries (-save-temps=obj)")
        for a in asms:
            _scan_unit(a, cmd, what, allow_calls)
        os.replace(prod, out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def build(force=False, verbose=False, extra_flags=(), scan=True):
    if not force and not needs_build():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)

    def compile_unit(u):
        src, obj = _src(u), _obj(u)
        if force or _unit_stale(u):
            variant = u.partition("@")[2]
            flags = FLAGS + VARIANT_FLAGS[variant] + list(extra_flags) + (["-Rpass-analysis=kernel-resource-usage"] if verbose else [])
            if verbose:
                print(" ".join([hipcc] + flags + ["-c", src, "-o", obj]), file=sys.stderr)
            if scan and src.endswith(".hip"):
                _compile_scanned(hipcc, flags, src, obj, os.path.basename(src) + ("@" + variant if variant else ""), allow_calls=variant not in NO_CALL_VARIANTS)
            else:
                subprocess.check_call([hipcc] + flags + ["-c", src, "-o", obj])
        return obj

    with ThreadPoolExecutor(max_workers=min(len(UNITS), os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_unit, UNITS))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB])
    selftest_if_gpu()
    return LIB


def selftest_if_gpu():
    """The known-answer self-tests (nuts_rs_amd/selftest.py) on the library just built, when this machine has a GPU — in a fresh process (the
    library of the building process may already be mapped): the two small runs on the wave / group / lane kernels, then EVERY instantiation of
    the one-chain-per-block kernels against its own known answer (349 runs, ~1 min).  Without a GPU (the cross-compiling
    build box) nothing runs and a line says so: smoke() and the first engine of each instantiation run them on the GPU box."""
    probe = ("import sys, torch\n"
             "sys.exit(0 if torch.cuda.is_available() else 3)\n")
    try:
        if subprocess.run([sys.executable, "-c", probe], capture_output=True, timeout=300).returncode != 0:
            print("nuts_rs_amd.build: no GPU here (or no torch): the known-answer self-tests of the built library were NOT run", file=sys.stderr)
            return False
    except Exception as e:          # noqa: BLE001
        print(f"nuts_rs_amd.build: GPU probe failed ({e!r}): the known-answer self-tests were NOT run", file=sys.stderr)
        return False
    code = ("import nuts_rs_amd.selftest as s; print(s.run(), 'self-test runs ok'); "
            "print(s.run_all(), 'kernel instantiations reproduce their known answers')")
    try:
        r = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(HERE, ".."), capture_output=True, text=True, timeout=1800,
                           env=dict(os.environ, NUTS_AMD_SELFTEST="0"))       # (run_all checks everything itself: no first-use checks inside it)
    except subprocess.TimeoutExpired:
        raise RuntimeError("the library was linked, but its known-answer self-test did not finish within 30 minutes on this GPU "
                           "(a hung kernel?): do not use this build") from None
    if r.returncode != 0:
        raise RuntimeError("the library just built FAILED its known-answer self-test on this GPU:\n" + r.stdout[-3000:] + r.stderr[-4000:])
    return True


def pick_tiling(dim, dims_per_lane=0, waves_per_chain=0):
    """(doubles per lane, waves per chain) the engine uses for `dim` — the same table as nm_pick_tiling."""
    for dpl, w in ((2, 1), (4, 1), (8, 1), (16, 1), (8, 2), (16, 2), (4, 4), (16, 4)):
        if dims_per_lane and dpl != dims_per_lane:
            continue
        if waves_per_chain and w != waves_per_chain:
            continue
        if dpl * 64 * w >= dim:
            return dpl, w
    raise ValueError(f"no tiling for dim {dim}")


def build_density_module(header, struct_name, dim, out, dims_per_lane=0, waves_per_chain=0, extra_flags=(), group_struct=None, lane_struct=None,
                         variants=()):
    """Compile a user density (a functor `struct_name` defined in `header`, see include/nuts_amd.h "User densities")
    with the engine's kernels into the module `out` for the tiling of `dim`.  Cross-compiles without a GPU (~20 s).
    variants: "low_rank" adds the kernels LowRankNutsSettings needs, "kinetic" those of the non-Euclidean trajectory kinds / MCLMC
    (each about doubles the build time)."""
    if dim > 4096:            # several blocks per chain: the cluster-mode kernels on the (16, 4) tiling; the density brings init_slice
        dpl, w = 16, 4
        extra_flags = list(extra_flags) + ["-DNM_CLUSTER_MODE=1"]
    else:
        dpl, w = pick_tiling(dim, dims_per_lane, waves_per_chain)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    header = os.path.abspath(header)
    if group_struct:          # the density's group form: several chains per wavefront for dim <= 64
        if dim > 64:
            raise ValueError("group forms exist for dim <= 64")
        extra_flags = list(extra_flags) + [f"-DNM_MODULE_GROUP_DENSITY={group_struct}", f"-DNM_MODULE_GS={8 if dim <= 16 else 16 if dim <= 32 else 32}"]
    if lane_struct:           # the density's lane form: one chain per lane for dim <= 10 (`template <int NP> struct ...`; the 8-pair kernel for dim 11 .. 16 was removed in round 5)
        if dim > 10:
            raise ValueError("lane forms exist for dim <= 10")
        extra_flags = list(extra_flags) + [f"-DNM_MODULE_LANE_DENSITY={lane_struct}"]
    # The special functions (nm::dexp / dlog / dlog1p, merge_math, ...) are INLINED in a module of a several-chains-per-wavefront form (a user functor
    # must not reach them through a call there: DESIGN §22, asm_scan.py's divergent-call rule) and, since round 5, in a module of a small tiling
    # (<= 4 doubles per lane) exactly as in the library's own units of those tilings: §22's fourth incident includes a dim-40 module whose
    # out-of-line build reported a wrong energy statistic while the inlined build of the same sources is bit-exact
    # (profiles/r05z_module_variants.txt), and a module is compiled on the USER's machine, where the engine's parity suite does not run.
    # Round 6: the defect behind those incidents is known (a VGPR spill placed above a join block's exec restore) and EVERY module
    # build — whatever its tiling, with or without calls — is scanned for it and repaired in the assembly (_scan_unit: the rules are in the
    # package, there is no build without them); the calls only made it likelier (SGPR spills around each call site).  The inlining rule stays.
    no_calls = bool(group_struct or lane_struct) or dpl <= 4
    if no_calls:
        extra_flags = list(extra_flags) + ["-DNM_DETMATH_INLINE=1"]
    vbits = (1 if "low_rank" in variants else 0) | (2 if "kinetic" in variants else 0)
    if vbits:
        if dim > 4096:
            raise ValueError("the low-rank / kinetic variants exist for dim <= 4096")
        extra_flags = list(extra_flags) + [f"-DNM_MODULE_VARIANTS={vbits}"]
    extra_flags = list(extra_flags) + os.environ.get("NM_MODULE_EXTRA_FLAGS", "").split()       # (tuning / bisecting builds of a module)
    flags = FLAGS + list(extra_flags) + [
        "-shared", f"-DNM_MODULE_DENSITY={struct_name}", f'-DNM_MODULE_HEADER="{header}"', f"-DNM_MODULE_DPL={dpl}",
        f"-DNM_MODULE_W={w}", "-I", CSRC, "-I", os.path.join(HERE, "..", "include")]
    # (the user's code is compiled into the same register-capped kernels: its assembly goes through the same scan as the engine's own)
    _compile_scanned(hipcc, flags, os.path.join(CSRC, "density_module.hip"), os.path.abspath(out), f"density module {struct_name}", link=True, allow_calls=not no_calls)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
