"""The game-kernel template instances of the built library, and a launch that reaches each of them (test helper, not a conftest).

Every result of the engine comes from one instance of ``fk_play_kernel`` (csrc/fk_kernels.h) or ``fk_play_hc_kernel`` (csrc/fk_play_hc.h).
``compiled_instances`` reads the instances out of the built shared object; ``MATRIX`` maps each of them to a ``Route``: the player count, the
table size and the ``set_option`` values under which the launch plan picks it, plus the flag form its tables must have.  The library reports
what it launched (``Engine.last_play_instance``) in the spelling used here: the demangled template name without its namespace.

The flag form of an instance (its ``MIXED`` argument) is chosen from the strategy table (csrc/farkle_hip.hip, ``mixed_form``):
``0u`` every flag shared by the whole table, ``49152u`` only require_both / favor_score differ, ``65280u`` any other flag differs.  In the two
narrow forms the shared flags come from the launch argument ``PlayArgs.uflags``, so ``flag_tables`` builds tables that share zeros as well
as ones.
"""
from __future__ import annotations

import re
from pathlib import Path
from typing import NamedTuple

import numpy as np

FLAG_NAMES = ("smart_five", "smart_one", "consider_score", "consider_dice", "require_both", "auto_hot_dice", "run_up_score", "favor_score")
FORMS = {"none": 0x0, "rb_fav": 0xC000, "all": 0xFF00}  # MIXED of the instance (csrc/farkle_hip.hip: MIXED_NONE / MIXED_RB_FAV / MIXED_ALL)

# ---- instances in the built library ----------------------------------------------------------------------------------------------

# Itanium mangling of a kernel in the sources' anonymous namespace, e.g.
#   _ZN12_GLOBAL__N_114fk_play_kernelILi768ELb1ELi6ELj49152ELb0ELb0ELi2EEEvNS_8PlayArgsE
# (the host-side launch stubs are ``..._GLOBAL__N_1<len>__device_stub__fk_play_kernel...``: another name, never matched)
_MANGLED = re.compile(rb"_ZN12_GLOBAL__N_1(\d+)(fk_play_kernel|fk_play_hc_kernel)I((?:L[ibj]n?\d+E)+)E")
_ARG = re.compile(r"L([ibj])(n?)(\d+)E")


def demangle_args(kind_args: str) -> list[str]:
    """``Li768ELb1ELj49152E`` -> ``["768", "true", "49152u"]`` (int, bool, unsigned as a demangler prints them)."""
    out = []
    for kind, neg, digits in _ARG.findall(kind_args):
        value = -int(digits) if neg else int(digits)
        out.append({"i": str(value), "b": "true" if value else "false", "j": f"{value}u"}[kind])
    return out


def instances_in_bytes(data: bytes) -> set[str]:
    found = set()
    for m in _MANGLED.finditer(data):
        length, name, args = int(m.group(1)), m.group(2).decode(), m.group(3).decode()
        if length != len(name):  # (a longer identifier that merely ends in the kernel's name)
            continue
        found.add(f"{name}<{', '.join(demangle_args(args))}>")
    return found


def compiled_instances(lib_path: str | Path) -> set[str]:
    """The game-kernel instances whose names the built library carries (kernel registration strings and the code object)."""
    return instances_in_bytes(Path(lib_path).read_bytes())


def instance_form(instance: str) -> str:
    """The flag form (a key of ``FORMS``) of an instance name."""
    args = instance[instance.index("<") + 1:-1].split(", ")
    mixed = int((args[3] if instance.startswith("fk_play_kernel<") else args[1]).rstrip("u"))
    return {v: k for k, v in FORMS.items()}[mixed]


def instance_shape(instance: str) -> str:
    """The instance name with its MIXED argument replaced by ``{m}`` (the key of ``SHAPES``)."""
    head, args = instance[:-1].split("<")
    parts = args.split(", ")
    parts[3 if head == "fk_play_kernel" else 1] = "{m}"
    return f"{head}<{', '.join(parts)}>"


# ---- routes ------------------------------------------------------------------------------------------------------------------------

class Route(NamedTuple):
    name: str     # short label: the pytest id
    entry: str    # "tournament" (fk_tournament_run*) or "h2h_blocks" (fk_h2h_run_blocks)
    k: int
    S: int        # table size, a multiple of k
    options: tuple  # (name, value) pairs for Engine.set_option; OPTION_DEFAULTS restores them
    form: str = ""  # filled in by MATRIX


OPTION_DEFAULTS = {"hot_cold": -1, "lean": -1, "block": 0, "state_store": -1, "use_lds_tally": -1, "uniform_flags": -1, "max_waves": 6}


def _lds(k, S, lean, block):
    # the LDS-record kernel, forced to one record layout and block size (hot / cold kernel off: it would take k >= 4)
    return Route(f"{'lean' if lean else 'full'}{block}_k{k}", "tournament", k, S,
                 (("hot_cold", 0), ("lean", 1 if lean else 0), ("block", block)))


def _hc(name, k, S):
    # the hot / cold kernel: the launch plan's own choice from four seats on (hot_cold -1); it never takes a launch with an LDS tally, so
    # one-batch calls go through result records
    return Route(name, "tournament", k, S, (("hot_cold", -1), ("use_lds_tally", 0)))


# one entry per template shape; every shape is compiled in all three flag forms
SHAPES = {
    "fk_play_kernel<1024, true, 4, {m}, false, false, 0>": _lds(2, 96, True, 1024),
    "fk_play_kernel<512, true, 4, {m}, false, false, 0>": _lds(3, 96, True, 512),
    "fk_play_kernel<256, true, 4, {m}, false, false, 0>": _lds(4, 96, True, 256),
    "fk_play_kernel<128, true, 4, {m}, false, false, 0>": _lds(6, 96, True, 128),
    "fk_play_kernel<64, true, 4, {m}, false, false, 0>": _lds(8, 96, True, 64),
    "fk_play_kernel<1024, false, 4, {m}, false, false, 0>": _lds(2, 96, False, 1024),
    "fk_play_kernel<512, false, 4, {m}, false, false, 0>": _lds(3, 96, False, 512),
    "fk_play_kernel<256, false, 4, {m}, false, false, 0>": _lds(4, 96, False, 256),
    "fk_play_kernel<128, false, 4, {m}, false, false, 0>": _lds(6, 96, False, 128),
    "fk_play_kernel<64, false, 4, {m}, false, false, 0>": _lds(8, 96, False, 64),
    "fk_play_kernel<768, true, 6, {m}, false, false, 0>": _lds(3, 96, True, 768),          # 768 threads, generic k
    "fk_play_kernel<768, true, 6, {m}, false, false, 2>": _lds(2, 96, True, 768),          # 768 threads, KC = 2
    "fk_play_kernel<768, true, 6, {m}, true, false, 0>": Route("state_store_k4", "tournament", 4, 96, (("hot_cold", 0), ("state_store", 1))),
    "fk_play_kernel<768, true, 6, {m}, false, true, 2>": Route("h2h_blocks", "h2h_blocks", 2, 96, ()),
    "fk_play_hc_kernel<320, {m}, false, 0, 6, false, true, 4>": _hc("hc_cold_in_lds_k4", 4, 96),
    "fk_play_hc_kernel<256, {m}, true, 5, 4, false, false, 6>": _hc("hc_k5", 5, 100),
    "fk_play_hc_kernel<512, {m}, true, 6, 4, false, false, 6>": _hc("hc_k6", 6, 96),
    "fk_play_hc_kernel<1024, {m}, true, 7, 4, false, false, 8>": _hc("hc_k7", 7, 98),
    "fk_play_hc_kernel<256, {m}, true, 8, 0, true, false, 8>": _hc("hc_k8", 8, 96),
    "fk_play_hc_kernel<768, {m}, true, 10, 3, false, false, 10>": _hc("hc_ns10_k10", 10, 100),
    "fk_play_hc_kernel<768, {m}, true, 12, 3, false, false, 12>": _hc("hc_ns12_k11", 11, 99),
}

MATRIX = {shape.format(m=f"{mixed}u"): route._replace(name=f"{route.name}-{form}", form=form)
          for shape, route in SHAPES.items() for form, mixed in FORMS.items()}


def matrix_gaps(compiled: set[str]) -> tuple[list[str], list[str]]:
    """(compiled instances without a route, routes whose instance is not compiled), sorted."""
    return sorted(compiled - set(MATRIX)), sorted(set(MATRIX) - compiled)


# ---- flag tables per form ----------------------------------------------------------------------------------------------------------

SCORE_THRESHOLDS = (0, 50, 100, 250, 300, 400, 500, 750, 1000, 1500, 2000, 3000)
DICE_THRESHOLDS = tuple(range(-1, 7))

# shared flag vectors of the scalar form: every flag is shared as 0 by one table and as 1 by another
NONE_FLAGS = {
    "zeros": {},
    "smart_five_only": {"smart_five": 1, "favor_score": 1},
    "consider_score_only": {"consider_score": 1},
    "consider_dice_only": {"consider_dice": 1, "auto_hot_dice": 1},
    "require_both": {"smart_five": 1, "smart_one": 1, "consider_score": 1, "consider_dice": 1, "require_both": 1, "run_up_score": 1},
    "both_considered": {"consider_score": 1, "consider_dice": 1, "auto_hot_dice": 1, "run_up_score": 1, "favor_score": 1},
    "ones": {name: 1 for name in FLAG_NAMES},
}


def table_form(table: np.ndarray) -> str:
    varying = {name for name in FLAG_NAMES if len(np.unique(table[name])) > 1}
    return "none" if not varying else "rb_fav" if varying <= {"require_both", "favor_score"} else "all"


def check_legal(table: np.ndarray) -> None:
    """The two invariants of the reference's ThresholdStrategy: smart_one => smart_five, require_both => both thresholds considered."""
    assert not (table["smart_one"] & ~table["smart_five"] & 1).any()
    assert not (table["require_both"] & ~(table["consider_score"] & table["consider_dice"]) & 1).any()


def _thresholds(S: int, seed: int) -> np.ndarray:
    from farkle_ii_amd.strategies import STRATEGY_DTYPE

    rng = np.random.default_rng(seed)
    t = np.zeros(S, dtype=STRATEGY_DTYPE)
    t["score_threshold"] = rng.permutation(np.resize(SCORE_THRESHOLDS, S))
    t["dice_threshold"] = rng.permutation(np.resize(DICE_THRESHOLDS, S))
    t["strategy_id"] = np.arange(S)
    return t


def _uniform(S: int, flags: dict, seed: int) -> np.ndarray:
    t = _thresholds(S, seed)
    for name in FLAG_NAMES:
        t[name] = flags.get(name, 0)
    return t


def _grid(S: int, seed: int, keep=None, **opts) -> np.ndarray:
    """A restricted grid of the reference's generator (the project's mirror of it), S of its strategies picked at random in grid order."""
    from farkle_ii_amd.strategies import generate_strategy_grid, pack_strategies

    strategies, _ = generate_strategy_grid(score_thresholds=list(SCORE_THRESHOLDS), dice_thresholds=list(DICE_THRESHOLDS), **opts)
    table = pack_strategies(strategies)
    if keep is not None:
        table = table[keep(table)]
    pick = np.sort(np.random.default_rng(seed).choice(len(table), S, replace=False))
    table = table[pick].copy()
    table["strategy_id"] = np.arange(S)
    return table


def _random_legal(S: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = _thresholds(S, seed)
    for name in ("smart_five", "consider_score", "consider_dice", "auto_hot_dice", "run_up_score", "favor_score"):
        t[name] = rng.integers(0, 2, S)
    t["smart_one"] = t["smart_five"] & rng.integers(0, 2, S).astype(np.uint8)
    t["require_both"] = t["consider_score"] & t["consider_dice"] & rng.integers(0, 2, S).astype(np.uint8)
    return t


def flag_tables(form: str, S: int) -> dict[str, np.ndarray]:
    """The strategy tables a route of flag form ``form`` plays (every one legal and of that form; thresholds spread over
    ``SCORE_THRESHOLDS`` and -1 .. 6 dice)."""
    tables = {}
    if form == "none":
        for i, (name, flags) in enumerate(NONE_FLAGS.items()):
            tables[name] = _uniform(S, flags, 100 + i)
    elif form == "rb_fav":
        fixed = {"consider_score_opts": [True], "consider_dice_opts": [True]}
        # (a) only favor_score varies (the generator varies it under smart_five with both thresholds considered); require_both,
        # smart_one, auto_hot_dice and run_up_score shared as 0
        tables["favor_only"] = _grid(S, 1, keep=lambda t: t["require_both"] == 0, smart_five_opts=[True], smart_one_opts=[False],
                                     auto_hot_dice_opts=[False], run_up_score_opts=[False], **fixed)
        # (b) a restricted grid as the generator makes it: require_both varies, smart_five / auto_hot_dice / run_up_score shared as 0
        # (without smart_five the generator only makes favor_score = SCORE) ...
        grid_b = _grid(S, 2, smart_five_opts=[False], smart_one_opts=[False], auto_hot_dice_opts=[False], run_up_score_opts=[False], **fixed)
        tables["require_both_grid"] = grid_b
        # ... and the same strategies with favor_score = DICE on every third one (legal: ThresholdStrategy checks only the two invariants)
        both = grid_b.copy()
        both["favor_score"][::3] = 0
        tables["require_both_and_favor"] = both
        # (c) g64-like: every shared flag set to 1
        tables["shared_ones"] = _grid(S, 3, smart_five_opts=[True], smart_one_opts=[True], auto_hot_dice_opts=[True], run_up_score_opts=[True],
                                      **fixed)
    else:
        tables["random"] = _random_legal(S, 4)
        only = _uniform(S, {"smart_five": 1, "consider_score": 1, "auto_hot_dice": 1, "favor_score": 1}, 5)
        only["run_up_score"] = np.arange(S) % 2  # the one flag outside require_both / favor_score that differs
        tables["run_up_only"] = only
    for name, t in tables.items():
        check_legal(t)
        assert table_form(t) == form, (form, name)
        assert len(t) == S
    return tables
