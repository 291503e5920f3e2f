"""Filtered planes, what only they have (their device code is branches of libmcrt_light_groups.so's and libmcrt_path_classes.so's resolve
kernels, whose generic checks are tests/test_side_libraries.py's): the flags against the C header with the structs' sizes and the ABI
version where they were, the binding's names, the two changed kernels inside the resources their notes record, and the gather's launch
guard. No GPU."""
import ctypes as C
import inspect
import os

import side_libraries as sl


def test_the_flags_are_the_headers_and_no_struct_grew(pkg, tmp_path):
    names = ["MCRT_LIGHT_GROUPS_SKY_PLANE", "MCRT_LIGHT_GROUPS_FILM", "MCRT_LIGHT_GROUPS_FILM_CLAMP", "MCRT_PATH_CLASSES_MAP", "MCRT_PATH_CLASSES_FILM",
             "MCRT_PATH_CLASSES_FILM_CLAMP", "MCRT_FILM_LANCZOS", "MCRT_ABI_VERSION"]
    got = sl.c_values(tmp_path, names + ["sizeof(mcrt_light_group_params)", "sizeof(mcrt_path_class_params)", "sizeof(mcrt_probe_params)"],
                      " ".join(["%u"] * len(names) + ["%zu"] * 3))
    assert got[:8] == [pkg.LIGHT_GROUPS_SKY_PLANE, pkg.LIGHT_GROUPS_FILM, pkg.LIGHT_GROUPS_FILM_CLAMP, pkg.PATH_CLASSES_MAP, pkg.PATH_CLASSES_FILM,
                       pkg.PATH_CLASSES_FILM_CLAMP, 6, pkg.ABI_VERSION] == [1, 2, 4, 1, 2, 4, 6, 2]
    assert got[8:] == [C.sizeof(pkg.LightGroupParams), C.sizeof(pkg.PathClassParams), C.sizeof(pkg.ProbeParams)] == [24, 16, 64]
    assert pkg.lib().mcrt_abi_version() == 2


def test_the_bindings_names_and_keywords_are_there(pkg):
    for name in ("render_light_groups", "render_light_groups_device", "render_path_classes", "render_path_classes_device", "render_lens"):
        parameters = inspect.signature(getattr(pkg.Context, name)).parameters
        assert parameters["film"].default is False and parameters["film_clamp"].default is False, name
    assert list(inspect.signature(pkg.Context.render_film).parameters)[:4] == ["self", "cam", "global_seed", "max_depth"]
    groups, _ = pkg.Context._light_group_params(None, 0, 3, 1, True, True)
    assert (groups.num_groups, groups.flags, groups.sky_plane, groups.max_depth) == (1, 1 | 2 | 4, 0, 3)
    assert pkg.Context._light_group_params(None, None, 0, None)[0].flags == 0
    classes = pkg.Context._path_class_params([0] * 8, 2, True, False)
    assert (classes.flags, classes.max_depth) == (1 | 2, 2) and pkg.Context._path_class_params(None, 0).flags == 0
    # the flags change no plane count
    L = pkg.lib()
    assert L.mcrt_light_group_planes(C.byref(groups)) == 1 and L.mcrt_path_class_planes(C.byref(classes)) == 1


def test_the_two_resolve_kernels_stay_within_their_resources(pkg):
    """The filtered planes are three more branches of lightGroupsResolveKernel and pathClassesResolveKernel: no kernel was added, both
    keep no LDS, no scratch and spill nothing, inside the rows their notes record, with eight waves a SIMD (64 VGPRs) as before."""
    pkg.lib()
    for stem, name, notes, regex in (("mcrt_light_groups", "lightGroupsResolveKernel", "NOTES_light_groups.md", r"lightGroups\w+Kernel"),
                                     ("mcrt_path_classes", "pathClassesResolveKernel", "NOTES_path_classes.md", r"pathClasses\w+Kernel")):
        kernels = {x["name"]: x for x in sl.kernels_of(os.path.join(sl.CSRC, "lib%s.so" % stem))}
        assert sorted(kernels) == sl.TABLE[stem]["kernels"]
        r = kernels[name]
        assert r["lds"] == 0 and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["agpr"] == 0 and r["max_wg"] == 256, r
        assert r["vgpr"] <= 64, r
        for word, bound in sl.recorded_resources(notes, regex)[name].items():
            assert r[word] <= bound, (name, word, r[word], bound)
        film = sl.recorded_resources("NOTES_film_gather.md", r"\w+ResolveKernel")[name]
        assert all(r[word] <= bound for word, bound in film.items()), (name, r, film)
