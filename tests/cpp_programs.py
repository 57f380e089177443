"""The one build rule of the C++ test programs under tests/cpp (a plain module,
not a conftest): build(name) compiles tests/cpp/<name>.cpp for gfx950 against
libdistjoin.so and returns the executable's path. The program is rebuilt when
it is missing or older than its source, any shared header of tests/cpp, any
public or csrc header, or the library."""
import glob
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
PKG = os.path.join(REPO, "distributed_join_amd")
LIB = os.path.join(PKG, "libdistjoin.so")
INCLUDE_DIRS = {"include": os.path.join(REPO, "include"), "csrc": os.path.join(PKG, "csrc")}


def _deps(src):
    deps = [src, LIB] + glob.glob(os.path.join(CPP, "*.hpp"))
    for pattern in ("include/*.hpp", "include/*.h", "distributed_join_amd/csrc/*.h",
                    "distributed_join_amd/csrc/*.hpp"):
        deps += glob.glob(os.path.join(REPO, pattern))
    return deps


def build(name, defines=(), include=("include",)):
    """Executable of tests/cpp/<name>.cpp. `include` names the product header
    folders it compiles against ("include": the public headers, "csrc": the
    library's own); a variant with `defines` gets a name of its own."""
    src = os.path.join(CPP, name + ".cpp")
    exe = os.path.join(CPP, "-".join([name] + [d.replace("=", "-") for d in defines]))
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe)
                                   for d in _deps(src)):
        return exe
    cmd = ["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", CPP]
    for d in include:
        cmd += ["-I", INCLUDE_DIRS[d]]
    cmd += ["-D" + d for d in defines]
    cmd += [src, "-o", exe, "-L", PKG, "-ldistjoin", "-Wl,-rpath,$ORIGIN/../../distributed_join_amd"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-6000:]
    return exe
