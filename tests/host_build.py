"""The only place in tests/ that starts a compiler: host builds of the per-lane headers under phc_amd/csrc (g++), stand-alone sanitizer programs (g++),
and C probes of include/phc_amd.h (gcc, so the header stays C)."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CSRC = os.path.join(ROOT, "phc_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _tmp():
    d = tempfile.mkdtemp(prefix="phc_host_build_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def shim(source, device_source):
    """ctypes.CDLL of the host build of tests/<source>.  `device_source` is the entry of phc_amd.build.SOURCES whose arithmetic the shim follows: the CPU-versus-GPU
    comparisons rest on both being compiled without contraction and without fast-math, so an entry that says otherwise is an error here."""
    from phc_amd.build import SOURCES
    flags = SOURCES[device_source]
    if "-ffp-contract=off" not in flags or "-ffast-math" in flags:
        raise RuntimeError(f"{source} follows {device_source}, whose flags in phc_amd/build.py are {flags}: it needs -ffp-contract=off and no -ffast-math")
    so = os.path.join(_tmp(), os.path.splitext(source)[0] + ".so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wno-comment", "-I", CSRC, os.path.join(TESTS, source), "-o", so], check=True)
    return ctypes.CDLL(so)


def run_sanitized(source):
    """Compile tests/<source> (a program with its own main) under AddressSanitizer + UBSan and run it as a child process: (returncode, stdout, stderr).
    Nothing is loaded into Python; the sanitizer runtimes are linked statically, so the program does not depend on the order of the process's shared libraries."""
    exe = os.path.join(_tmp(), os.path.splitext(source)[0])
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-std=c++17", "-I", CSRC, os.path.join(TESTS, source), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


def header_values(*exprs):
    """The integer C expressions `exprs` (sizeof(phc_x_t), offsetof(phc_x_t, f), PHC_MACRO ...) evaluated against include/phc_amd.h, as ints, in order."""
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "phc_amd.h"\nint main(void){\n' + "".join(f'printf("%lld\\n", (long long)({e}));\n' for e in exprs) + "return 0;}\n"
    with tempfile.TemporaryDirectory(dir=_tmp()) as d:
        c, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        with open(c, "w") as f:
            f.write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    vals = [int(x) for x in out.split()]
    assert len(vals) == len(exprs)
    return vals
