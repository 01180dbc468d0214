"""The one g++ build of the CPU harnesses (tests/harness/<name>.cpp over the headers of csrc/): every *_cases.build_harness() and the
sanitizer tests call this; they keep their ctypes prototypes.  (The `harness` fixture of tests/conftest.py has a copy of its own for
fr_math_harness: that file is one of the yardsticks and is not edited.)"""
import glob
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDIR = os.path.join(ROOT, "tests", "harness")
CSRC = os.path.join(ROOT, "fisher-nerf-customized_amd", "csrc")
EXACT = ("-ffp-contract=off",)                  # arithmetic rounds as written; the expected values of the CPU tests depend on these flags
EXACT_FMA = EXACT + ("-mfma",)                  # and fmaf() is the instruction (the harnesses whose headers call it)


def compile_shared(src, so, extra_flags=()):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", *extra_flags, "-o", so, src])


def shared(name, extra_flags=EXACT_FMA):
    """tests/harness/<name>.cpp -> tests/harness/lib<name>.so, rebuilt when it is missing or older than the .cpp or ANY header of csrc/
    or include/ (no per-harness dependency list to fall behind the #includes); returns the path"""
    src, so = os.path.join(HDIR, name + ".cpp"), os.path.join(HDIR, "lib" + name + ".so")
    deps = [src] + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        compile_shared(src, so, extra_flags)
    return so


def sanitized_program(name, define, tmp_path):
    """tests/harness/<name>.cpp as a program of its own (-D<define> gives it a main) under -fsanitize=address,undefined, run once;
    returns the completed process.  Nothing is preloaded: the sanitizer runtime is linked into the program."""
    exe = str(tmp_path / (name + "_asan"))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D" + define, "-o", exe, os.path.join(HDIR, name + ".cpp")])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)
