"""tests/emu_build.py, the one builder of the emulation libraries: when it builds and when it does not, on a three-line source with a
one-line header in a scratch directory; and on the real tree, that a library's prerequisites are what the compiler read."""
import ctypes as C
import os
import shutil

from emu_build import build_emu, prerequisites


def _mtime(path):
    return os.stat(path).st_mtime_ns


def test_the_builder_builds_when_something_changed_and_only_then(tmp_path):
    header, source, out = tmp_path / "answer.hpp", tmp_path / "answer_emu.cpp", str(tmp_path / "_build")
    header.write_text("#define ANSWER 42\n")
    text = '#include "answer.hpp"\nextern "C" int answer() { return ANSWER + EXTRA; }\n'
    source.write_text(text)

    def build(extra=0):
        return build_emu(str(source), flags=["-DEXTRA=%d" % extra], opt="-O0", build_dir=out)

    lib = build()  # the first call builds
    assert lib == os.path.join(out, "libanswer_emu.so") and C.CDLL(lib).answer() == 42
    assert str(header) in prerequisites(lib) and str(source) in prerequisites(lib)
    assert [f for f in os.listdir(out) if ".tmp" in f] == []
    first = _mtime(lib)
    assert build() == lib and _mtime(lib) == first  # the second does not
    os.utime(header, ns=(first + 10 ** 6, first + 10 ** 6))  # a header newer than the library
    build()
    second = _mtime(lib)
    assert second > first and build() == lib and _mtime(lib) == second
    build(extra=1)  # a changed flag, every file as old as it was
    third = _mtime(lib)
    assert third > second
    shutil.copy(lib, lib + ".copy")  # (loaded under another name: the process keeps what it loaded under the first)
    assert C.CDLL(lib + ".copy").answer() == 43
    assert build(extra=1) == lib and _mtime(lib) == third
    # a prerequisite that is gone: the source no longer includes it and is as old as before, so that nothing else makes the library stale
    old = os.stat(source)
    source.write_text(text.replace('#include "answer.hpp"', "#define ANSWER 7"))
    os.utime(source, ns=(old.st_atime_ns, old.st_mtime_ns))
    assert build(extra=1) == lib and _mtime(lib) == third  # (the text alone does not rebuild: the mtimes decide)
    header.unlink()
    build(extra=1)
    assert _mtime(lib) > third and str(header) not in prerequisites(lib)


def test_the_denoise_filters_depend_on_the_skeleton_they_share():
    """Both a-trous filters live in csrc/mcrt_atrous.hpp; the lists typed by hand did not name it."""
    for source in ("denoise_emu.cpp", "denoise_var_emu.cpp"):
        names = [os.path.basename(p) for p in prerequisites(build_emu(source))]
        assert "mcrt_atrous.hpp" in names and source in names and "mcrt.h" in names, (source, names)
