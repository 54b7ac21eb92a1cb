"""Test infrastructure (pytest plugin): which error returns of the library's host units (rcw_api.hip, rcw_rules.hip, rcw_step.hip,
rcw_comm.hip) does a run provoke?

    RCW_LIBRARY=$PWD/raycastworlds.jl_amd/lib/librcw_hip_dev.so PYTHONPATH=tests python -m pytest tests -m gpu -q -p failsite_plugin

Every default load then takes the development build, whose fail() records its source file and line (rcw_dev_fail_unit names the
units, rcw_dev_fail_sites hands out one unit's lines), written as file:line in the report (both exports: the development build
only); at the end the explicit `fail(` sites never taken are listed in gpurun_out/failcov_<FAILCOV_TAG>.txt.  (The calls of the
rank scripts, the examples and the plain-C harness run in other processes and are not counted.)"""
import ctypes as C, os, re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def pytest_sessionfinish(session, exitstatus):
    from raycastworlds_jl_amd import _capi
    lib = C.CDLL(_capi.DEV_LIB_PATH)            # (the same loaded object: dlopen returns the resident one)
    lib.rcw_dev_fail_unit.restype = C.c_char_p
    hit, src, sites = set(), {}, []
    unit = 0
    while (name := lib.rcw_dev_fail_unit(unit)) is not None:
        name = name.decode()
        buf = (C.c_ubyte * 4096)()
        n = lib.rcw_dev_fail_sites(unit, buf, 4096)
        hit |= {(name, i) for i in range(n) if buf[i]}
        lines = open(os.path.join(ROOT, "raycastworlds.jl_amd", "csrc", name)).read().splitlines()
        for i, l in enumerate(lines):
            src[(name, i + 1)] = l
            if re.search(r"\bfail\(|RCW_HIP\(|RCW_NCCL\(", l) and not l.lstrip().startswith(("#define", "//")):
                sites.append((name, i + 1))
        unit += 1
    tag = os.environ.get("FAILCOV_TAG", "run")
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", f"failcov_{tag}.txt"), "w") as f:
        expl = [s for s in sites if "fail(" in src[s]]
        f.write(f"{len(hit)} lines recorded; explicit fail( sites: {len(expl)}, of them taken: {len([s for s in expl if s in hit])}\n")
        f.write("explicit sites never taken:\n")
        for s in expl:
            if s not in hit:
                f.write(f"  {s[0]}:{s[1]}: {src[s].strip()[:170]}\n")
        f.write("HIP / RCCL call sites whose failure branch was taken:\n")
        for s in sites:
            if s in hit and "fail(" not in src[s]:
                f.write(f"  {s[0]}:{s[1]}: {src[s].strip()[:170]}\n")
