"""Every game-kernel instance the built library holds has a test route (tests/kernel_instances.py: MATRIX), and every route names an
instance that is built.  A new template instance without a route, or a route whose instance left the library, fails here on any machine;
tests/test_kernel_instances_gpu.py plays every route against the oracle."""
from __future__ import annotations

from collections import defaultdict

import kernel_instances as ki


def _library():
    from farkle_ii_amd import backend

    return backend.build_library()


def test_every_compiled_instance_has_a_route_and_every_route_is_compiled():
    compiled = ki.compiled_instances(_library())
    no_route, not_compiled = ki.matrix_gaps(compiled)
    assert not no_route and not not_compiled, (
        "game-kernel instances without a route in tests/kernel_instances.py:\n  " + "\n  ".join(no_route) +
        "\nroutes whose instance the library does not hold:\n  " + "\n  ".join(not_compiled))
    assert len(compiled) == 63  # 14 shapes of fk_play_kernel + 7 of fk_play_hc_kernel, three flag forms each


def test_every_shape_is_compiled_in_all_three_flag_forms():
    forms = defaultdict(set)
    for inst in ki.compiled_instances(_library()):
        forms[ki.instance_shape(inst)].add(ki.instance_form(inst))
    incomplete = {shape: sorted(f) for shape, f in forms.items() if f != set(ki.FORMS)}
    assert not incomplete, incomplete
    assert set(forms) == set(ki.SHAPES)


def test_instance_names_are_read_from_the_mangled_strings():
    """The parser against hand-made mangled names: all three argument kinds, the host-side launch stubs skipped, a longer identifier
    that ends in a kernel's name skipped."""
    blob = (b"\0_ZN12_GLOBAL__N_114fk_play_kernelILi768ELb1ELi6ELj49152ELb0ELb0ELi2EEEvNS_8PlayArgsE\0"
            b"_ZN12_GLOBAL__N_129__device_stub__fk_play_kernelILi64ELb0ELi4ELj0ELb0ELb0ELi0EEEvNS_8PlayArgsE\0"
            b"_ZN12_GLOBAL__N_117fk_play_hc_kernelILi768ELj65280ELb1ELi12ELi3ELb0ELb0ELi12EEEvNS_8PlayArgsE\0"
            b"_ZN12_GLOBAL__N_117my_fk_play_kernelILi1ELb0ELi4ELj0ELb0ELb0ELi0EEEvNS_8PlayArgsE\0")
    assert ki.instances_in_bytes(blob) == {"fk_play_kernel<768, true, 6, 49152u, false, false, 2>",
                                           "fk_play_hc_kernel<768, 65280u, true, 12, 3, false, false, 12>"}
    assert ki.instance_form("fk_play_hc_kernel<768, 65280u, true, 12, 3, false, false, 12>") == "all"
    assert ki.instance_form("fk_play_kernel<768, true, 6, 0u, true, false, 0>") == "none"


def test_routes_are_well_formed_and_flag_tables_have_their_form():
    for inst, route in ki.MATRIX.items():
        assert route.form == ki.instance_form(inst), inst
        assert route.S % route.k == 0 and 96 <= route.S <= 100, route
        assert set(dict(route.options)) <= set(ki.OPTION_DEFAULTS), route
    assert len({r.name for r in ki.MATRIX.values()}) == len(ki.MATRIX)
    for form in ki.FORMS:
        for S in {r.S for r in ki.MATRIX.values()}:
            tables = ki.flag_tables(form, S)  # (checks legality and the form of every table itself)
            assert len(tables) == {"none": 7, "rb_fav": 4, "all": 2}[form]
    # the scalar form's tables share every flag as 0 in one table and as 1 in another
    for name in ki.FLAG_NAMES:
        assert {int(t[name][0]) for t in ki.flag_tables("none", 96).values()} == {0, 1}, name
