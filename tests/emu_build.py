"""The one builder of the CPU tier's emulation libraries (tests/emu/*.cpp -> tests/emu/_build/lib*.so). The prerequisites of a library are
what the compiler says they are (-MD -MF, read the way monte-carlo-ray-tracer_amd/build.py reads its own), and the command line is
recorded next to the library, so that a changed flag rebuilds as a changed header does. A plain helper module like side_libraries.py and
oracle_lib.py - no fixtures, no hooks. (tests/conftest.py's own loaders do not come through here: DESIGN.md "Emulation tier".)"""
import os
import subprocess

TESTS = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(TESTS, "emu")
BUILD = os.path.join(EMU, "_build")


def prerequisites(lib):
    """What the compiler read to build `lib` (its .d file, a make rule), or None when there is no such file."""
    try:
        text = open(os.path.splitext(lib)[0] + ".d").read()
    except OSError:
        return None
    text = text.replace("\\\n", " ")
    return [t for t in text.split(":", 1)[1].split() if t] if ":" in text else None


def _stale(lib, command):
    deps = prerequisites(lib)
    if deps is None or not os.path.exists(lib):
        return True
    try:
        if open(os.path.splitext(lib)[0] + ".cmd").read() != command:
            return True
        t = os.stat(lib).st_mtime_ns
        return any(os.stat(d).st_mtime_ns > t for d in deps)
    except OSError:  # no recorded command, or a prerequisite that is gone
        return True


def build_emu(source, lib_name=None, flags=(), link=(), opt="-O2", fp_contract="-ffp-contract=off", build_dir=BUILD):
    """`source` (a path, or a file name under tests/emu/) built into build_dir/<lib_name> (default: lib<source's stem>.so) when that
    library is stale; -> its path. The command is g++ -std=c++17 <opt> <fp_contract> -fPIC -shared <flags> -MD -MF <lib>.d -o <lib>
    <source> <link>; fp_contract=None leaves that flag out. The library is built aside and renamed: parallel workers stay safe."""
    source = os.path.join(EMU, source)  # (an absolute path stays what it is)
    stem = os.path.join(build_dir, os.path.splitext(lib_name or "lib" + os.path.basename(source))[0])
    lib, tmp = stem + ".so", "%s.%d.tmp" % (stem, os.getpid())
    head = ["g++", "-std=c++17", opt] + ([fp_contract] if fp_contract else []) + ["-fPIC", "-shared"] + list(flags)
    command = " ".join(head + ["-o", lib, source] + list(link))
    if _stale(lib, command):
        os.makedirs(build_dir, exist_ok=True)
        subprocess.check_call(head + ["-MD", "-MF", tmp + ".d", "-o", tmp + ".so", source] + list(link))
        with open(tmp + ".cmd", "w") as f:
            f.write(command)
        for ext in (".d", ".cmd", ".so"):  # the library last: whoever finds it finds its two files
            os.replace(tmp + ext, stem + ext)
    return lib
