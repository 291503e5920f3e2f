"""The kernels of every image pass are a code object of their own, beside the render path's. For each row of tests/side_libraries.py:
lib<stem>.so holds exactly the row's kernels, within the row's resources; no other library on disk - libmcrt_hip.so, the render path's
device code listed function by function in tests/golden/device_code_hashes.json, its tolerance build, the other side libraries - holds a
kernel the row's rule names; both main libraries find the library next to themselves (RUNPATH $ORIGIN); the pass's calls are exported. And
over all of them: the rows are build.py's PASSES, every library on disk has a row, no kernel name occurs in two libraries."""
import importlib
import os

import pytest

import side_libraries as sl

STEMS = list(sl.TABLE)


def _lib(stem):
    return os.path.join(sl.CSRC, "lib%s.so" % stem)


def _main_libs():
    assert os.path.exists(os.path.join(sl.CSRC, sl.MAIN_LIBS[0]))
    return [os.path.join(sl.CSRC, lib) for lib in sl.MAIN_LIBS if not lib.endswith("_tol.so") or os.path.exists(os.path.join(sl.CSRC, lib))]  # (MCRT_SKIP_TOLERANCE_BUILD=1 builds)


def test_the_rows_are_the_passes_of_the_build():
    build = importlib.import_module("monte-carlo-ray-tracer_amd.build")
    assert tuple(sl.TABLE) == tuple(build.PASSES)
    assert [lib for lib, _ in build.SIDE_LIBS] == [_lib(stem) for stem in STEMS]
    assert all(stem + "_host.hip" in build.TUS for stem in STEMS)


def test_every_side_library_on_disk_has_a_row(pkg):
    pkg.lib()
    assert [f for f in sl.libraries_on_disk() if f not in sl.MAIN_LIBS] == sorted("lib%s.so" % stem for stem in STEMS)


def test_the_main_library_holds_the_render_path(pkg):
    pkg.lib()
    assert len(sl.kernels_of(os.path.join(sl.CSRC, sl.MAIN_LIBS[0]))) > 300


@pytest.mark.parametrize("stem", STEMS)
def test_the_library_holds_exactly_its_kernels_within_their_resources(pkg, stem):
    pkg.lib()
    row = sl.TABLE[stem]
    kernels = {k["name"]: k for k in sl.kernels_of(_lib(stem))}
    assert sorted(kernels) == row["kernels"]
    recorded = sl.recorded_resources(*row["notes"]) if row["notes"] else None
    if recorded is not None:
        assert sorted(recorded) == row["kernels"]
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (name, k)
        if name not in row["sgpr_spill_allowed"]:  # (spilled SGPRs go to lanes of a VGPR, not to memory)
            assert k["sgpr_spill"] == 0, (name, k)
        if name in row["max_wg"]:
            assert k["max_wg"] == row["max_wg"][name], (name, k)
        if recorded is not None:
            for word, bound in recorded[name].items():
                assert k[word] <= bound, (name, word, k[word], bound)
        if row["lds"] is not None:
            assert k["lds"] == row["lds"].get(name, 0), (name, k)


def test_no_kernel_name_occurs_in_two_libraries(pkg):
    """... over every library on disk; the tolerance build of the main library holds the main library's names and is told apart from it."""
    pkg.lib()
    where = {}
    for lib in sl.libraries_on_disk():
        names = {k["name"] for k in sl.kernels_of(os.path.join(sl.CSRC, lib))}
        assert names, lib
        for name in names:
            where.setdefault(name, set()).add(lib)
    assert not {name: sorted(libs) for name, libs in where.items() if len(libs) > 1 and libs != set(sl.MAIN_LIBS)}


@pytest.mark.parametrize("stem", STEMS)
def test_no_other_library_holds_a_kernel_of(pkg, stem):
    pkg.lib()
    row = sl.TABLE[stem]
    others = [f for f in sl.libraries_on_disk() if f != "lib%s.so" % stem and f not in row["skip"]]
    assert set(sl.MAIN_LIBS[:1]) <= set(others) and len(others) >= len(STEMS) - len(row["skip"])
    for lib in others:
        names = [k["name"] for k in sl.kernels_of(os.path.join(sl.CSRC, lib))]
        assert names and not [n for n in names if sl.foreign(row["foreign"], n, row["kernels"])], lib
    assert all(sl.foreign(row["foreign"], n, row["kernels"]) for n in row["kernels"])  # (the rule does name the pass's own kernels)


@pytest.mark.parametrize("stem", STEMS)
def test_the_main_libraries_find_the_library_next_to_themselves(stem):
    for path in _main_libs():
        dyn = sl.dynamic_section(path)
        assert "[lib%s.so]" % stem in [l.split()[-1] for l in dyn.splitlines() if "NEEDED" in l], path
        assert any("$ORIGIN" in l for l in dyn.splitlines() if "RUNPATH" in l or "RPATH" in l), path
    if sl.TABLE[stem]["no_libz"]:
        for path in _main_libs() + [_lib(stem)]:
            needed = [l for l in sl.dynamic_section(path).splitlines() if "NEEDED" in l]
            assert not [l for l in needed if "libz" in l], (path, needed)


@pytest.mark.parametrize("stem", STEMS)
def test_the_calls_are_exported_and_the_abi_version_stays(pkg, stem):
    L = pkg.lib()
    row = sl.TABLE[stem]
    for name in row["calls"]:
        assert hasattr(L, name), name
    assert L.mcrt_abi_version() == 2
    for name in row["attributes"]:
        assert hasattr(pkg, name), name
    for name in row["methods"]:
        assert hasattr(pkg.Context, name), name
