"""ctypes binding of the C-ABI library (``include/farkle_hip.h`` -> ``farkle_ii_amd/libfarkle_hip.so``).

This is the only door from Python into the simulation: there is no CPU fallback.  If the shared
library has not been built, or no HIP device is usable, constructing an :class:`Engine` raises.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
import subprocess
from pathlib import Path

import numpy as np

from .strategies import STRATEGY_DTYPE

PKG_DIR = Path(__file__).resolve().parent
# FARKLE_HIP_LIB: load another build of the same C-ABI (A/B timing of kernel variants); the default is the in-tree library
LIB_PATH = Path(os.environ.get("FARKLE_HIP_LIB", PKG_DIR / "libfarkle_hip.so"))
SRC_DIR = PKG_DIR / "csrc"
HEADER = PKG_DIR.parent / "include" / "farkle_hip.h"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

COORD_DTYPE = np.dtype(
    [("purpose", "<u4"), ("pad", "<u4"), ("root_seed", "<u8"), ("k", "<u8"), ("shuffle_index", "<u8"),
     ("pair_id", "<u8"), ("order", "<u8"), ("game_index", "<u8"), ("seat_index", "<u8"), ("replicate_index", "<u8")]
)
OVERRIDE_DTYPE = np.dtype(
    [("root_seed", "<u8"), ("a", "<u8"), ("b", "<u8"), ("k_or_order", "<u4"), ("max_rounds", "<u4")]
)
SEAT_DTYPE = np.dtype(
    [("score", "<i4"), ("strategy", "<i4"), ("farkles", "<u2"), ("rolls", "<u2"), ("n_turns", "<u2"),
     ("highest_turn", "<u2"), ("smart_five_uses", "<u2"), ("n_smart_five_dice", "<u2"), ("smart_one_uses", "<u2"),
     ("n_smart_one_dice", "<u2"), ("hot_dice", "<u2"), ("rank", "u1"), ("hit_max_rounds", "u1")]
)
H2H_BLOCK_DTYPE = np.dtype(
    [("seats", STRATEGY_DTYPE, (2,)), ("pair_id", "<u8"), ("order", "<u4"), ("pad", "<u4"), ("target", "<u8"),
     ("max_attempts", "<u8"), ("state", "<u8", (5,))]
)
# fk_roll_event, include/farkle_hip.h: one roll of a traced game (fk_trace_games; decoders in farkle_ii_amd/trace.py)
EVENT_DTYPE = np.dtype(
    [("dice", "<u4"), ("turn_score", "<i4"), ("points", "<u2"), ("round", "<u2"), ("seat", "u1"), ("used_left", "u1"),
     ("discards", "u1"), ("flags", "u1")]
)
# fk_rr_pair_row, include/farkle_hip.h: one pair of the round-robin inference (fk_rr_inference; frames in farkle_ii_amd/rr_inference.py)
RR_PAIR_ROW_DTYPE = np.dtype(
    [("pair_id", "<u8"), ("games_attempted", "<i8"), ("games_completed", "<i8"), ("games_safety_limit", "<i8"), ("n_completed_required", "<i8"),
     ("n_ab", "<i8"), ("n_ba", "<i8"), ("seat1_a_wins_ab", "<i8"), ("seat1_b_wins_ba", "<i8"), ("seat2_a_wins_ba", "<i8"), ("balanced_a_wins", "<i8"),
     ("holm_order", "<i8"), ("completion_game_rate", "<f8"), ("q_ab", "<f8"), ("q_ba", "<f8"), ("raw_order_rate_difference", "<f8"), ("d_ab", "<f8"),
     ("score_null_proportion", "<f8"), ("score_z", "<f8"), ("score_p_value", "<f8"), ("ordinary_d_low", "<f8"), ("ordinary_d_high", "<f8"),
     ("simultaneous_d_low", "<f8"), ("simultaneous_d_high", "<f8"), ("balanced_a_win_rate", "<f8"), ("holm_adjusted_p", "<f8"),
     ("strategy_a", "<u4"), ("strategy_b", "<u4"), ("flags", "u1"), ("decision_class", "u1"), ("pad", "u1", (6,))]
)
# fk_rr_root_row / fk_rr_agreement_row, include/farkle_hip.h: one (root, pair) and one pair of the per-root diagnostics
# (fk_rr_root_diagnostics; frames in farkle_ii_amd/rr_root_diagnostics.py)
RR_ROOT_ROW_DTYPE = np.dtype(
    [("pair_id", "<u8"), ("games_attempted", "<i8"), ("games_completed", "<i8"), ("games_safety_limit", "<i8"), ("n_ab", "<i8"), ("n_ba", "<i8"),
     ("seat1_a_wins_ab", "<i8"), ("seat1_b_wins_ba", "<i8"), ("holm_order", "<i8"), ("completion_game_rate", "<f8"), ("q_ab", "<f8"), ("q_ba", "<f8"),
     ("d_ab", "<f8"), ("score_null_proportion", "<f8"), ("score_z", "<f8"), ("score_p_value", "<f8"), ("ordinary_d_low", "<f8"),
     ("ordinary_d_high", "<f8"), ("holm_adjusted_p", "<f8"), ("strategy_a", "<u4"), ("strategy_b", "<u4"), ("flags", "u1"),
     ("diagnostic_decision", "u1"), ("pad", "u1", (6,))]
)
RR_AGREEMENT_ROW_DTYPE = np.dtype(
    [("pair_id", "<u8"), ("root_a_d_ab", "<f8"), ("root_b_d_ab", "<f8"), ("effect_discrepancy_a_minus_b", "<f8"), ("absolute_effect_discrepancy", "<f8"),
     ("strategy_a", "<u4"), ("strategy_b", "<u4"), ("root_a_decision", "u1"), ("root_b_decision", "u1"), ("flags", "u1"), ("pad", "u1", (5,))]
)
RR_MAX_ROOTS = 2       # FK_RR_MAX_ROOTS
RR_AGREE_COLS = 12     # FK_RR_AGREE_COLS
# fk_dom_node / fk_dom_extreme, include/farkle_hip.h: the dominance graphs of a round robin (fk_dominance_graph; frames in farkle_ii_amd/dominance.py)
DOM_NODE_DTYPE = np.dtype(
    [("component", "<u4", (2,)), ("component_size", "<u4", (2,)), ("front", "<u4", (2,)), ("cycle_length", "<u4", (2,)), ("wins", "<u4", (2,)),
     ("losses", "<u4", (2,)), ("rate_count", "<u8"), ("rate_mean", "<f8")]
)
DOM_EXTREME_DTYPE = np.dtype(
    [("strongest_winner", "<u4"), ("strongest_loser", "<u4"), ("weakest_winner", "<u4"), ("weakest_loser", "<u4"), ("strongest_distance", "<f8"),
     ("weakest_distance", "<f8")]
)
DOM_MAX_N = 8192       # FK_DOM_MAX_N
RR_CLASSES = 7         # FK_RR_CLASSES
AGREE_COUNTS = 11      # FK_AGREE_COUNTS
AGREE_NO_RANK = 0      # FK_AGREE_NO_RANK
CONCORDANCE_COUNTS = 5  # FK_CONCORDANCE_COUNTS
CONCORDANCE_MAX_M = 65536  # FK_CONCORDANCE_MAX_M
CONCORDANCE_TILE = 256  # FK_CONCORDANCE_TILE
RR_STRATEGY_COLS = 12  # FK_RR_STRATEGY_COLS
# fk_power_cell, include/farkle_hip.h: one (sample size, scenario) cell of fk_score_power_scan (the plan in farkle_ii_amd/h2h_power.py)
POWER_CELL_DTYPE = np.dtype([("n", "<i4"), ("reserved", "<i4"), ("q_ab", "<f8"), ("q_ba", "<f8")])
POWER_MAX_N = 1048576  # FK_POWER_MAX_N
POWER_LDS_MAX_N = 3071  # FK_POWER_LDS_MAX_N
ROOT_WINDOW_MAX_CELLS = 256  # FK_ROOT_WINDOW_MAX_CELLS
# fk_root_window_estimates: the planes of its two outputs, in their order
ROOT_WINDOW_TOTALS = ("wins", "exposures", "completed", "safety", "losses", "positive_batches")
ROOT_WINDOW_SUMS = ("sum_w2", "sum_we", "sum_e2")
TALLY_COLS = 26
LAG_COLS = 11  # FK_LAG_COLS: pairs | win: sx sy sxx syy sxy | n_rounds: sx sy sxx syy sxy
SEAT_STAT_COLS = 31
SEAT_RATIO_COLS = 4  # FK_SEAT_RATIO_COLS: sum / sum of squares of score / n_turns, of score / n_rounds (float64, (shuffle, game, seat) order)
SEAT_STAT_NAMES = ("exposures", "completed_exposures", "safety_limit_exposures", "wins", "final_score_sum", "final_score_square_sum",
                   "n_turns_sum", "n_turns_square_sum", "turn_round_mismatch_count", "turn_minus_rounds_sum",
                   "turn_minus_rounds_square_sum") + tuple(
    f"{name}_{kind}" for name in ("rank", "loss_margin", "rolls", "farkles", "highest_turn", "hot_dice", "smart_five_uses",
                                   "n_smart_five_dice", "smart_one_uses", "n_smart_one_dice") for kind in ("sum", "square_sum"))
# tally columns (run_tournament.py:109-121, 165-195)
COL_WINS, COL_ATTEMPTED, COL_COMPLETED, COL_SAFETY, COL_SUMS, COL_SQ_SUMS = 0, 1, 2, 3, 4, 15

FK_ERR_ROLL_LIMIT, FK_ERR_ARG, FK_ERR_COUNTER_OVERFLOW, FK_ERR_HIP, FK_ERR_NO_DEVICE, FK_ERR_COMM, FK_ERR_IO = -1, -2, -3, -4, -5, -6, -7
COMM_ID_BYTES = 128


def row_dtype(k: int) -> np.dtype:
    """Structured dtype of one game row: 4-byte header + k 28-byte seat records."""
    return np.dtype([("n_rounds", "<u2"), ("status", "u1"), ("winner_seat", "i1"), ("seats", SEAT_DTYPE, (k,))])


class _RrInferenceParams(C.Structure):  # fk_rr_inference_params
    _fields_ = [("family_alpha", C.c_double), ("practical_delta", C.c_double), ("delta_equivalence", C.c_double),
                ("min_candidate_completion_rate", C.c_double), ("critical_ordinary", C.c_double), ("critical_simultaneous", C.c_double),
                ("family_pair_count", C.c_uint64)]


class _DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("arch", C.c_char * 32), ("compute_units", C.c_int32), ("clock_mhz", C.c_int32),
                ("wavefront_size", C.c_int32), ("lds_bytes_per_cu", C.c_int32), ("hbm_bytes", C.c_uint64)]


class _Timing(C.Structure):
    _fields_ = [("perm_ms", C.c_float), ("seed_ms", C.c_float), ("play_ms", C.c_float), ("total_ms", C.c_float),
                ("play_launches", C.c_int32), ("play_block", C.c_int32), ("play_grid", C.c_int32),
                ("play_lds_bytes", C.c_int32), ("games", C.c_int64), ("prefetched_chunks", C.c_int32), ("play_clock_mhz", C.c_int32),
                ("play_block_end_p50_ms", C.c_float), ("play_block_end_max_ms", C.c_float), ("play_mixed_flags", C.c_int32),
                ("ho_handovers", C.c_int64), ("ho_lanes_served", C.c_int64), ("ho_trips", C.c_int64),
                ("ho_waiting_lane_trips", C.c_int64), ("ho_rolling_lane_trips", C.c_int64), ("ho_waves", C.c_int64)]


class FarkleHipError(RuntimeError):
    """Raised for every non-zero return of the C-ABI; ``code`` is the FK_ERR_* value."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


def hip_sources() -> list[Path]:
    return [SRC_DIR / "farkle_hip.hip"]


VARIANTS = {"detour": ["-DFK_FORCE_DETOUR=4"]}  # test builds: libfarkle_hip_<variant>.so beside the product library
# measuring builds, compiled on demand (build_library(variant=...)) and never by build(): "count" fills fk_timing's ho_* hand-over counts
TOOL_VARIANTS = {"count": ["-DFK_COUNT_HANDOVER"]}


def library_path(variant: str | None = None) -> Path:
    return LIB_PATH if not variant else LIB_PATH.with_name(f"libfarkle_hip_{variant}.so")


def build_library(force: bool = False, verbose: bool = False, variant: str | None = None) -> Path:
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU).  ``variant``: a test build with extra
    definitions (``VARIANTS``), never loaded by the product."""
    out = library_path(variant)
    deps = sorted(p for p in SRC_DIR.iterdir() if p.is_file()) + [HEADER]  # (a new header cannot be forgotten)
    if out.exists() and not force and all(out.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return out
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", *({**VARIANTS, **TOOL_VARIANTS}[variant] if variant else []), "-o", str(out),
           *[str(s) for s in hip_sources()]]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(" ".join(cmd))
        print(res.stdout, res.stderr)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed ({res.returncode}): {res.stderr[-2000:]}")
    return out


_BY_VALUE = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "double": C.c_double}
_RETURNS = {"int": C.c_int, "void": None, "size_t": C.c_size_t, "const char *": C.c_char_p}
_PROTOTYPE_START = re.compile(r"^(?:int|void|size_t|const char \*)\s*\*?fk_\w+\(", re.M)
_PROTOTYPE = re.compile(r"^(int|void|size_t|const char \*)\s*(fk_\w+)\(([^;{}()]*)\);", re.M)


def parse_signatures(header_text: str) -> dict:
    """``{name: (restype, argtypes)}`` of every ``fk_*`` prototype in the text of a header: by-value parameters by ``_BY_VALUE``, ``const char *``
    as c_char_p, every other pointer or array parameter as c_void_p (which takes ``_p(array)``, ``byref(...)``, string buffers, ctypes arrays and
    None).  A by-value type without a mapping, or a line that begins like a prototype and is not matched as one, raises: none is skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header_text, flags=re.S)
    found = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        argtypes = []
        for param in (" ".join(p.split()) for p in params.split(",") if p.strip() not in ("", "void")):
            if "*" in param or "[" in param:
                argtypes.append(C.c_char_p if re.fullmatch(r"const char \* ?\w+", param) else C.c_void_p)
            elif param.rsplit(" ", 1)[0] in _BY_VALUE:
                argtypes.append(_BY_VALUE[param.rsplit(" ", 1)[0]])
            else:
                raise ValueError(f"{name}: no ctypes type for the by-value parameter `{param}`")
        found[name] = (_RETURNS[ret], argtypes)
    if len(found) != len(_PROTOTYPE_START.findall(text)):
        raise ValueError(f"{len(_PROTOTYPE_START.findall(text))} lines begin like a prototype, {len(found)} distinct prototypes were parsed")
    return found


@functools.lru_cache(maxsize=None)
def signatures() -> dict:
    """``parse_signatures`` of ``include/farkle_hip.h``: the declared entry points, and what ``load_library`` sets on each."""
    return parse_signatures(HEADER.read_text())


_libs: dict = {}


def load_library(variant: str | None = None) -> C.CDLL:
    """dlopen the in-tree library; loud failure when it has not been built."""
    if variant not in _libs:
        path = library_path(variant)
        if not path.exists():
            raise FileNotFoundError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the simulation path)")
        lib = C.CDLL(str(path))
        for name, (restype, argtypes) in signatures().items():
            fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = restype, argtypes
        _libs[variant] = lib
    return _libs[variant]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


CENSUS_TABLES = ("roll_cells", "strategy_dice", "strategy_turns", "turn_hist")
CENSUS_ROLL_SHAPE = (6, 61, 7)  # dice rolled - 1, raw score / 50, raw dice used


class _Census(C.Structure):  # fk_census
    _fields_ = [("turn_bins", C.c_int32), ("roll_cells", C.c_void_p), ("strategy_dice", C.c_void_p), ("strategy_turns", C.c_void_p),
                ("turn_hist", C.c_void_p)]


def _census_tables(S: int, turn_bins: int) -> tuple[dict, _Census]:
    """Zeroed int64 tables of a census call and the ``fk_census`` that points at them."""
    shapes = (CENSUS_ROLL_SHAPE, (S, 6, 3), (S, 3), (S, max(int(turn_bins), 0)))
    tables = {name: np.zeros(shape, dtype=np.int64) for name, shape in zip(CENSUS_TABLES, shapes)}
    return tables, _Census(int(turn_bins), *(tables[name].ctypes.data for name in CENSUS_TABLES))


def row_columns_bytes(k: int, games_per_shuffle: int) -> int:
    """``fk_row_columns_bytes``: bytes of one shuffle's column image."""
    return int(load_library().fk_row_columns_bytes(k, games_per_shuffle))


class _ShardJob(C.Structure):
    _fields_ = [("k", C.c_int32), ("games_per_shuffle", C.c_int32), ("n_shuffles", C.c_int32), ("threads", C.c_int32), ("atomic", C.c_int32),
                ("rng_purpose_namespace", C.c_int32), ("root_seed", C.c_uint64), ("shuffle_index", C.c_void_p), ("shuffle_seed", C.c_void_p),
                ("batch_id", C.c_void_p), ("game_seed", C.c_void_p), ("columns", C.c_void_p), ("shard_stride", C.c_size_t),
                ("directory", C.c_char_p), ("footer_head", C.c_char_p), ("footer_head_len", C.c_size_t), ("footer_kv", C.c_char_p),
                ("footer_kv_len", C.c_size_t), ("footer_orders", C.c_char_p), ("footer_orders_len", C.c_size_t), ("leaf_type", C.c_void_p),
                ("leaf_paths", C.c_char_p), ("n_leaves", C.c_int32), ("side_body", C.POINTER(C.c_char_p)), ("side_full", C.POINTER(C.c_char_p)),
                ("side_directory", C.c_char_p)]


def write_row_shards_native(row_dir, k: int, root_seed: int, columns: np.ndarray, shuffle_index, shuffle_seed, batch_id, game_seeds,
                            rng_purpose_namespace: int, *, threads: int = 1, atomic: bool = True, sidecar: dict | None = None) -> dict:
    """``fk_write_row_shards``: the row-shard files of ``columns`` (``[n_shuffles][stride]`` column images) in ``row_dir``, written by
    ``threads`` host threads of the library.  Returns ``byte_length`` int64 ``[n]``, ``sha256`` uint8 ``[n][32]`` and — with a contract-v3
    ``sidecar`` template (``contract_v3.SimulationContract.shard_template``) — ``sidecar_sha256``."""
    return prepare_row_shards_native(row_dir, k, root_seed, columns, shuffle_index, shuffle_seed, batch_id, game_seeds, rng_purpose_namespace,
                                     threads=threads, atomic=atomic, sidecar=sidecar)()


def prepare_row_shards_native(row_dir, k: int, root_seed: int, columns: np.ndarray, shuffle_index, shuffle_seed, batch_id, game_seeds,
                              rng_purpose_namespace: int, *, threads: int = 1, atomic: bool = True, sidecar: dict | None = None):
    """``write_row_shards_native`` in two steps: the job is checked and laid out here; the returned callable makes the one library call
    (``columns`` may be filled in between: `farkle run` hands the callable to its shard thread, which then holds the interpreter lock
    for a few bytecodes per launch group)."""
    from .parquet_template import shard_footer_template

    lib = load_library()
    columns = np.ascontiguousarray(columns, dtype=np.uint8)
    n = len(columns)
    stride = columns.shape[1] if columns.ndim == 2 else 0
    gps = np.asarray(game_seeds).size // max(n, 1)
    tpl = shard_footer_template(k)
    sh = np.ascontiguousarray(shuffle_index, dtype=np.int64)
    seeds = np.ascontiguousarray(shuffle_seed, dtype=np.int64)
    batch = np.ascontiguousarray(batch_id, dtype=np.int32)
    gs = np.ascontiguousarray(game_seeds, dtype=np.uint32).reshape(-1)
    if not (len(sh) == len(seeds) == len(batch) == n) or gs.size != n * gps or stride < row_columns_bytes(k, gps):
        raise ValueError("shard job arrays disagree about the number of shuffles / games per shuffle")
    leaf_type = np.ascontiguousarray(tpl["leaf_type"], dtype=np.int32)
    leaf_paths = b"".join(b"".join(part.encode("utf-8") + b"\0" for part in path) + b"\0" for path in tpl["leaf_paths"])
    job = _ShardJob(k=k, games_per_shuffle=gps, n_shuffles=n, threads=max(1, int(threads)), atomic=1 if atomic else 0,
                    rng_purpose_namespace=int(rng_purpose_namespace), root_seed=int(root_seed), shuffle_index=sh.ctypes.data,
                    shuffle_seed=seeds.ctypes.data, batch_id=batch.ctypes.data, game_seed=gs.ctypes.data, columns=columns.ctypes.data,
                    shard_stride=stride, directory=os.fspath(row_dir).encode("utf-8"), footer_head=tpl["footer_head"],
                    footer_head_len=len(tpl["footer_head"]), footer_kv=tpl["footer_kv"], footer_kv_len=len(tpl["footer_kv"]),
                    footer_orders=tpl["footer_orders"], footer_orders_len=len(tpl["footer_orders"]), leaf_type=leaf_type.ctypes.data,
                    leaf_paths=leaf_paths, n_leaves=len(leaf_type))
    side_sha = None
    if sidecar is not None:
        body = (C.c_char_p * 4)(*[piece.encode("utf-8") for piece in sidecar["body"]])
        full = (C.c_char_p * 5)(*[piece.encode("utf-8") for piece in sidecar["full"]])
        job.side_body, job.side_full, job.side_directory = body, full, sidecar["directory"].encode("utf-8")
        side_sha = np.zeros((n, 32), dtype=np.uint8)
    sizes = np.zeros(n, dtype=np.int64)
    sha = np.zeros((n, 32), dtype=np.uint8)
    err = C.create_string_buffer(512)
    keep = (columns, sh, seeds, batch, gs, leaf_type, leaf_paths, tpl, sidecar)  # what the job points into

    def run() -> dict:
        rc = lib.fk_write_row_shards(C.byref(job), _p(sizes), _p(sha), _p(side_sha), err, len(err))
        if rc != 0:
            raise OSError(f"fk_write_row_shards failed ({rc}): {err.value.decode('utf-8', 'replace')}")
        return {"byte_length": sizes, "sha256": sha, "sidecar_sha256": side_sha}

    run.keep = keep  # (alive as long as the callable is)
    return run


def make_overrides(items) -> np.ndarray:
    """items: (root_seed, a, b, k_or_order, max_rounds) tuples -> fk_override[]."""
    items = list(items)
    out = np.zeros(len(items), dtype=OVERRIDE_DTYPE)
    for i, it in enumerate(items):
        out[i] = tuple(int(v) for v in it)
    return out


def make_coords(purpose, root_seed, k, shuffle_index=0, pair_id=0, order=0, game_index=0, n: int | None = None) -> np.ndarray:
    """Broadcast scalars/arrays into an fk_coord[] (seat_index = replicate_index = 0)."""
    arrs = [np.atleast_1d(np.asarray(v)) for v in (purpose, root_seed, k, shuffle_index, pair_id, order, game_index)]
    n = max(len(a) for a in arrs) if n is None else n
    out = np.zeros(n, dtype=COORD_DTYPE)
    for name, a in zip(("purpose", "root_seed", "k", "shuffle_index", "pair_id", "order", "game_index"), arrs):
        out[name] = a
    return out


# the game-stat outputs of fk_tournament_run_game_stats / fk_tournament_run_rare_events, in the entries' argument order
GAME_STAT_ARRAYS = ("strategy_counts", "strategy_rounds", "strategy_runner", "strategy_spread", "game_counts", "game_rounds", "game_runner")


class Engine:
    """One context (HIP stream + device workspace) on one GPU."""

    def __init__(self, device: int = 0, variant: str | None = None):
        self._lib = load_library(variant)  # (variant: a test build of the library, backend.VARIANTS)
        self._ctx = C.c_void_p()
        self._rr_n = 0  # the table size of the resident round-robin pair counts (0: none)
        rc = self._lib.fk_init(device, C.byref(self._ctx))
        if rc != 0:
            self._ctx = C.c_void_p()
            names = {FK_ERR_NO_DEVICE: "no usable HIP device (this engine has no CPU fallback)", FK_ERR_ARG: "bad device ordinal",
                     FK_ERR_HIP: "HIP runtime failure during fk_init"}
            raise FarkleHipError(rc, f"fk_init({device}) failed: {names.get(rc, rc)}")
        self.device = device
        self.comm_world = 1
        self.comm_rank = 0

    # -- plumbing -------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.fk_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int) -> None:
        if rc != 0:
            msg = self._lib.fk_last_error(self._ctx)
            raise FarkleHipError(rc, (msg or b"").decode() or f"error {rc}")

    def set_option(self, name: str, value: int) -> None:
        self._check(self._lib.fk_set_option(self._ctx, name.encode(), int(value)))

    def device_info(self) -> dict:
        info = _DeviceInfo()
        self._check(self._lib.fk_get_device_info(self._ctx, C.byref(info)))
        return {"name": info.name.decode(), "arch": info.arch.decode(), "compute_units": info.compute_units,
                "clock_mhz": info.clock_mhz, "wavefront_size": info.wavefront_size,
                "lds_bytes_per_cu": info.lds_bytes_per_cu, "hbm_bytes": int(info.hbm_bytes)}

    def timing(self) -> dict:
        t = _Timing()
        self._check(self._lib.fk_get_timing(self._ctx, C.byref(t)))
        return {f: getattr(t, f) for f, _ in _Timing._fields_}

    def last_play_instance(self) -> str:
        """``fk_last_play_instance``: the game-kernel template instance the last tournament / game-list / H2H call launched last
        (after a replay: the replay's), e.g. ``fk_play_kernel<768, true, 6, 49152u, false, false, 2>``; ``""`` when it launched none."""
        return (self._lib.fk_last_play_instance(self._ctx) or b"").decode()

    # -- hot path ------------------------------------------------------------------------
    @staticmethod
    def _setup(table, shuffle_begin, shuffle_end, shuffles_per_batch, overrides):
        """What every ``tournament*`` method starts with: the packed table, S, the shuffles of the range (an empty or reversed range
        counts none), the batch size, the batches, the override array and a zeroed tally ``[max(n_batches, 1)][S][TALLY_COLS]``."""
        table = np.ascontiguousarray(table, dtype=STRATEGY_DTYPE)
        S = len(table)
        n_sh = max(int(shuffle_end) - int(shuffle_begin), 0)
        spb = max(n_sh if not shuffles_per_batch else int(shuffles_per_batch), 1)
        n_batches = (n_sh + spb - 1) // spb
        ov = np.ascontiguousarray(overrides if overrides is not None else np.zeros(0, dtype=OVERRIDE_DTYPE), dtype=OVERRIDE_DTYPE)
        return table, S, n_sh, spb, n_batches, ov, np.zeros((max(n_batches, 1), S, TALLY_COLS), dtype=np.int64)

    def _lead(self, table, S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, ov, tally) -> tuple:
        """The thirteen leading arguments of every ``fk_tournament_run*`` entry."""
        return self._ctx, _p(table), S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, _p(ov), len(ov), _p(tally)

    @staticmethod
    def _game_stat_arrays(S, rb, mb) -> dict:
        """The seven int64 game-stat outputs (the entries take them in the order of ``GAME_STAT_ARRAYS``)."""
        shapes = ((S, 4), (S, rb), (S, mb), (S, mb), 4, rb, mb)
        return {name: np.zeros(shape, np.int64) for name, shape in zip(GAME_STAT_ARRAYS, shapes)}

    @staticmethod
    def _lag_arrays(lags, S, n_sh) -> tuple:
        """The lag list as int32, m = min(max lag, n_shuffles), and zeroed ``lag_sums`` / ``lag_head`` / ``lag_tail`` of the lag entries."""
        lags = np.ascontiguousarray(list(lags), dtype=np.int32)
        m = min(int(lags.max()) if len(lags) else 0, n_sh)
        return lags, m, np.zeros((S, len(lags), LAG_COLS), np.int64), np.zeros((max(m, 1), S), np.uint16), np.zeros((max(m, 1), S), np.uint16)

    def tournament(self, table: np.ndarray, k: int, root_seed: int, shuffle_begin: int, shuffle_end: int,
                   shuffles_per_batch: int | None = None, target_score: int = 10_000, max_rounds: int = 200,
                   overrides: np.ndarray | None = None, want_rows: bool = False, want_perms: bool = False,
                   want_seat_stats: bool = False, rows_out: np.ndarray | None = None, want_seat_ratios: bool = True) -> dict:
        """All games of shuffles ``[shuffle_begin, shuffle_end)``: per-batch tallies (+ rows / permutations / the all-seat
        integer statistics ``[n_batches][S][SEAT_STAT_COLS]``, columns ``SEAT_STAT_NAMES``, with the four float64 ratio sums
        ``seat_ratio_sums [n_batches][S][SEAT_RATIO_COLS]`` of the same table unless ``want_seat_ratios`` is off: they are one
        sequential sum per (batch, strategy), which a caller that only reads the integer columns need not wait for)."""
        table, S, n_sh, spb, n_batches, ov, tally = self._setup(table, shuffle_begin, shuffle_end, shuffles_per_batch, overrides)
        gps = S // k if k > 0 else 0
        rows = None
        if want_rows:
            n_rows = n_sh * gps
            if rows_out is not None:  # e.g. a page-locked buffer from pinned_empty(): rows cross PCIe by DMA while the next chunk plays
                if rows_out.dtype != row_dtype(k) or len(rows_out) < n_rows or not rows_out.flags["C_CONTIGUOUS"]:
                    raise ValueError("rows_out must be a contiguous array of row_dtype(k) with room for every game")
                rows = rows_out[:n_rows]
            else:
                rows = np.zeros(n_rows, dtype=row_dtype(k))
        perms = np.zeros((n_sh, S), dtype=np.int32) if want_perms else None
        stats = np.zeros((max(n_batches, 1), S, SEAT_STAT_COLS), dtype=np.int64) if want_seat_stats else None
        ratios = np.zeros((max(n_batches, 1), S, SEAT_RATIO_COLS), dtype=np.float64) if want_seat_stats and want_seat_ratios else None
        lead = self._lead(table, S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, ov, tally)
        if ratios is not None:  # the all-player accumulators: 31 integer sums + the four float64 sums in (shuffle, game, seat) order
            self._check(self._lib.fk_tournament_run_all_player(*lead, _p(rows), _p(perms), _p(stats), _p(ratios)))
        else:
            self._check(self._lib.fk_tournament_run_stats(*lead, _p(rows), _p(perms), _p(stats)))
        return {"tally": tally[:n_batches], "rows": rows, "perms": perms,
                "seat_stats": None if stats is None else stats[:n_batches],
                "seat_ratio_sums": None if ratios is None else ratios[:n_batches]}

    def tournament_game_stats(self, table: np.ndarray, k: int, root_seed: int, shuffle_begin: int, shuffle_end: int,
                              shuffles_per_batch: int | None = None, target_score: int = 10_000, max_rounds: int = 200,
                              overrides: np.ndarray | None = None, rare_target_score: int = 10_000, want_seat_stats: bool = False,
                              spill_capacity: int = 4096) -> dict:
        """``tournament`` + the game-stats stage's sufficient statistics of the range (``fk_tournament_run_game_stats``), with the
        all-player arrays of ``tournament(..., want_seat_stats=True)`` from the same launch when ``want_seat_stats``.  ``game_stats``
        holds int64 ``strategy_counts [S][4]``, ``strategy_rounds [S][R + 1]`` (R = max(max_rounds, every override)),
        ``strategy_runner`` / ``strategy_spread [S][M]`` (margin / 50), ``game_counts [4]``, ``game_rounds [R + 1]``, ``game_runner [M]``:
        the device's spill entries already merged (``game_stats.merge_spills``)."""
        from .game_stats import DEVICE_MARGIN_BINS, DEVICE_ROUNDS_BINS, merge_spills

        table, S, n_sh, spb, n_batches, ov, tally = self._setup(table, shuffle_begin, shuffle_end, shuffles_per_batch, overrides)
        R = max([int(max_rounds)] + [int(v) for v in ov["max_rounds"]])
        rb, mb = min(R + 1, DEVICE_ROUNDS_BINS), DEVICE_MARGIN_BINS
        capacity = max(int(spill_capacity), 0)
        while True:
            tally[:] = 0
            stats = np.zeros((max(n_batches, 1), S, SEAT_STAT_COLS), dtype=np.int64) if want_seat_stats else None
            ratios = np.zeros((max(n_batches, 1), S, SEAT_RATIO_COLS), dtype=np.float64) if want_seat_stats else None
            g = self._game_stat_arrays(S, rb, mb)
            spill = np.zeros((max(capacity, 1), 3), dtype=np.int32)
            spilled = C.c_int64(0)
            rc = self._lib.fk_tournament_run_game_stats(
                *self._lead(table, S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, ov, tally),
                None, None, _p(stats), _p(ratios), rare_target_score, rb, mb, *(_p(g[name]) for name in GAME_STAT_ARRAYS), capacity,
                C.byref(spilled), _p(spill))
            if rc == FK_ERR_ARG and spilled.value > capacity:  # more values outside the windows than room: once more with room for all
                capacity = int(spilled.value)
                continue
            self._check(rc)
            break
        return {"tally": tally[:n_batches], "seat_stats": None if stats is None else stats[:n_batches],
                "seat_ratio_sums": None if ratios is None else ratios[:n_batches], "spilled": int(spilled.value),
                "game_stats": merge_spills(g, spill[:spilled.value], R + 1)}

    def tournament_rare_events(self, table: np.ndarray, k: int, root_seed: int, shuffle_begin: int, shuffle_end: int,
                               shuffles_per_batch: int | None = None, target_score: int = 10_000, max_rounds: int = 200,
                               overrides: np.ndarray | None = None, rare_target_score: int = 10_000, thresholds=(),
                               want_events: bool = True, want_seat_stats: bool = False, spill_capacity: int = 4096,
                               event_capacity: int = 65_536, retry: bool = True) -> dict:
        """``tournament_game_stats`` (the same keys, the same values) + ``rare_events`` (``fk_tournament_run_rare_events``): int64
        ``strategy_second [S][B]`` / ``game_second [B]`` (second-highest seat score / 50 of every game with k >= 2, spills merged)
        and the games that are rare events under ``rare_target_score`` / ``thresholds`` (at most eight, points), in ascending
        (shuffle, game) order: ``event_head`` uint32 ``[n][4]``, ``event_seats`` uint16 ``[n][k]`` (``rare_events.event_fields``).
        ``want_events=False`` is the histograms-only call (``thresholds`` must be empty).  A list that is too small is an
        ``FK_ERR_ARG`` carrying the size it needs: the range is played again with that room unless ``retry`` is off."""
        from .game_stats import DEVICE_MARGIN_BINS, DEVICE_ROUNDS_BINS, merge_spills
        from .rare_events import DEVICE_SECOND_BINS, MAX_THRESHOLDS, SPILL_SECOND, merge_second_spills

        table, S, n_sh, spb, n_batches, ov, tally = self._setup(table, shuffle_begin, shuffle_end, shuffles_per_batch, overrides)
        thr = np.ascontiguousarray([int(t) for t in thresholds], dtype=np.int32)
        if len(thr) > MAX_THRESHOLDS:
            raise ValueError(f"at most {MAX_THRESHOLDS} margin thresholds per call, got {len(thr)}")
        if not want_events and len(thr):
            raise ValueError("the histograms-only call takes no thresholds")
        R = max([int(max_rounds)] + [int(v) for v in ov["max_rounds"]])
        rb, mb, sb = min(R + 1, DEVICE_ROUNDS_BINS), DEVICE_MARGIN_BINS, DEVICE_SECOND_BINS
        capacity = max(int(spill_capacity), 0)
        ev_cap = max(int(event_capacity), 0) if want_events else 0
        attempts = 0
        while True:
            attempts += 1
            tally[:] = 0
            stats = np.zeros((max(n_batches, 1), S, SEAT_STAT_COLS), dtype=np.int64) if want_seat_stats else None
            ratios = np.zeros((max(n_batches, 1), S, SEAT_RATIO_COLS), dtype=np.float64) if want_seat_stats else None
            g = self._game_stat_arrays(S, rb, mb)
            s_second, g_second = np.zeros((S, sb), np.int64), np.zeros(sb, np.int64)
            spill = np.zeros((max(capacity, 1), 3), dtype=np.int32)
            spilled, n_events = C.c_int64(0), C.c_int64(0)
            head = np.zeros((max(ev_cap, 1), 4), dtype=np.uint32) if want_events else None
            seats = np.zeros((max(ev_cap, 1), max(int(k), 1)), dtype=np.uint16) if want_events else None
            rc = self._lib.fk_tournament_run_rare_events(
                *self._lead(table, S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, ov, tally),
                None, None, _p(stats), _p(ratios), rare_target_score, rb, mb, *(_p(g[name]) for name in GAME_STAT_ARRAYS), capacity,
                C.byref(spilled), _p(spill), sb, _p(s_second), _p(g_second), len(thr), _p(thr) if len(thr) else None, ev_cap,
                C.byref(n_events), _p(head), _p(seats))
            short = spilled.value > capacity or n_events.value > ev_cap
            if rc == FK_ERR_ARG and short and retry:  # once more with room for all
                capacity, ev_cap = max(capacity, int(spilled.value)), max(ev_cap, int(n_events.value))
                continue
            try:
                self._check(rc)
            except FarkleHipError as err:  # (what the lists need travels with the error)
                err.events_needed, err.spill_needed = int(n_events.value), int(spilled.value)
                raise
            break
        entries = spill[:spilled.value]
        second = entries[:, 1] == SPILL_SECOND
        s_second, g_second = merge_second_spills(s_second, g_second, entries[second])
        n = int(n_events.value)
        return {"tally": tally[:n_batches], "seat_stats": None if stats is None else stats[:n_batches],
                "seat_ratio_sums": None if ratios is None else ratios[:n_batches], "spilled": int(spilled.value),
                "game_stats": merge_spills(g, entries[~second], R + 1), "attempts": attempts,
                "rare_events": {"strategy_second": s_second, "game_second": g_second, "events": n,
                                "event_head": head[:n].copy() if want_events else np.zeros((0, 4), np.uint32),
                                "event_seats": seats[:n].copy() if want_events else np.zeros((0, max(int(k), 1)), np.uint16)}}

    def tournament_seat_counts(self, table: np.ndarray, k: int, root_seed: int, shuffle_begin: int, shuffle_end: int,
                               shuffles_per_batch: int | None = None, target_score: int = 10_000, max_rounds: int = 200,
                               overrides: np.ndarray | None = None, strategy_ids=None, want_mirrored: bool = False,
                               pair_capacity: int = 65_536, retry: bool = True) -> dict:
        """``tournament`` (the same tally) + the seat-analysis stage's counts of the range (``fk_tournament_run_seat_counts``):
        ``seat_counts`` int64 ``[n_batches][S][k][3]`` = wins, completed exposures, safety-limit exposures per batch, table index and
        seat.  ``want_mirrored`` (k = 2, unique ``strategy_ids``, ``shuffle_begin`` on a batch boundary): ``pair_index`` uint16
        ``[n][2]`` (table indices, the lower ID first) and ``pair_sums`` int64 ``[n][6]`` (``seat_analysis.PAIR_COLUMNS``) in
        ascending ID order.  A pair list that is too small is an ``FK_ERR_ARG`` carrying the size it needs: the range is played
        once more with that room unless ``retry`` is off."""
        from .seat_analysis import id_ranks

        table, S, n_sh, spb, n_batches, ov, tally = self._setup(table, shuffle_begin, shuffle_end, shuffles_per_batch, overrides)
        rank = None
        if want_mirrored:
            if strategy_ids is None:
                raise ValueError("mirrored pairs need strategy_ids")
            rank = id_ranks(strategy_ids, S)
        capacity = max(int(pair_capacity), 0) if want_mirrored else 0
        attempts = 0
        while True:
            attempts += 1
            tally[:] = 0
            counts = np.zeros((max(n_batches, 1), S, max(int(k), 1), 3), dtype=np.int64)
            n_pairs = C.c_int64(0)
            index = np.zeros((max(capacity, 1), 2), dtype=np.uint16) if want_mirrored else None
            sums = np.zeros((max(capacity, 1), 6), dtype=np.int64) if want_mirrored else None
            rc = self._lib.fk_tournament_run_seat_counts(
                *self._lead(table, S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, ov, tally),
                _p(counts), _p(rank), capacity, C.byref(n_pairs) if want_mirrored else None, _p(index), _p(sums))
            if rc == FK_ERR_ARG and want_mirrored and n_pairs.value > capacity and retry and attempts == 1:
                capacity = int(n_pairs.value)
                continue
            try:
                self._check(rc)
            except FarkleHipError as err:  # (what the list needs travels with the error)
                err.pairs_needed = int(n_pairs.value)
                raise
            break
        n = int(n_pairs.value)
        return {"tally": tally[:n_batches], "seat_counts": counts[:n_batches], "attempts": attempts,
                "pair_index": index[:n].copy() if want_mirrored else None, "pair_sums": sums[:n].copy() if want_mirrored else None}

    def tournament_columns(self, table: np.ndarray, k: int, root_seed: int, shuffle_begin: int, shuffle_end: int, strategy_ids,
                           shuffles_per_batch: int | None = None, target_score: int = 10_000, max_rounds: int = 200,
                           overrides: np.ndarray | None = None, columns_out: np.ndarray | None = None, async_rows: bool = False,
                           shuffle_seeds_out: np.ndarray | None = None, game_seeds_out: np.ndarray | None = None) -> dict:
        """``tournament`` with the rows as per-shuffle COLUMN IMAGES (``fk_tournament_run_columns``): ``columns`` uint8
        ``[n_shuffles][fk_row_columns_bytes(k, S / k)]`` — what ``write_row_shards_native`` frames as the row-shard Parquet files.
        ``async_rows``: return when the last copy to the host is queued; read ``columns`` after ``rows_wait(result["rows_event"])``.
        ``shuffle_seeds_out`` uint32 ``[n_shuffles]`` / ``game_seeds_out`` uint32 ``[n_shuffles * S / k]``: also filled, complete on return
        (``fk_tournament_run_columns_seeds``: the fingerprints a shard's manifest record and its game_seed column carry)."""
        table, S, n_sh, spb, n_batches, ov, tally = self._setup(table, shuffle_begin, shuffle_end, shuffles_per_batch, overrides)
        ids = np.ascontiguousarray(strategy_ids, dtype=np.int32)
        if len(ids) != S:
            raise ValueError("strategy_ids must name every strategy of the table")
        stride = row_columns_bytes(k, S // k)
        if columns_out is not None:
            if columns_out.dtype != np.uint8 or columns_out.size < n_sh * stride or not columns_out.flags["C_CONTIGUOUS"]:
                raise ValueError("columns_out must be a contiguous uint8 array with room for every shuffle's image")
            columns = columns_out.reshape(-1)[:n_sh * stride].reshape(n_sh, stride)
        else:
            columns = np.zeros((n_sh, stride), dtype=np.uint8)
        rows_event = None
        if n_sh:
            if async_rows:
                self.set_option("rows_async", 1)
            try:
                for name, arr, want in (("shuffle_seeds_out", shuffle_seeds_out, n_sh), ("game_seeds_out", game_seeds_out, n_sh * (S // k))):
                    if arr is not None and (arr.dtype != np.uint32 or arr.size != want or not arr.flags["C_CONTIGUOUS"]):
                        raise ValueError(f"{name} must be a contiguous uint32 array of {want} elements")
                self._run_columns(table, S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, ov, tally, ids, columns,
                                  shuffle_seeds_out, game_seeds_out)
                if async_rows:
                    rows_event = self.get_option("rows_event")
            finally:
                if async_rows:
                    self.set_option("rows_async", 0)
        return {"tally": tally[:n_batches], "columns": columns, "rows_event": rows_event}

    def rows_wait(self, slot: int) -> None:
        """``fk_rows_wait``: the column images of the ``async_rows`` call that reported ``rows_event == slot`` are in the host buffer."""
        self._check(self._lib.fk_rows_wait(self._ctx, slot))

    columns_with_seeds = True  # (tournament_columns takes shuffle_seeds_out / game_seeds_out)

    def _run_columns(self, table, S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, ov, tally, ids, columns,
                     shuffle_seeds=None, game_seeds=None) -> None:
        args = (*self._lead(table, S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, ov, tally), _p(ids), _p(columns))
        if shuffle_seeds is None and game_seeds is None:
            self._check(self._lib.fk_tournament_run_columns(*args))
        else:
            self._check(self._lib.fk_tournament_run_columns_seeds(*args, _p(shuffle_seeds), _p(game_seeds)))

    def tournament_lags(self, table: np.ndarray, k: int, root_seed: int, shuffle_begin: int, shuffle_end: int, lags,
                        shuffles_per_batch: int | None = None, target_score: int = 10_000, max_rounds: int = 200,
                        overrides: np.ndarray | None = None) -> dict:
        """``tournament`` + the lag sufficient statistics of the strategy family (``fk_tournament_run_lags``):
        ``lag_sums [S][n_lags][LAG_COLS]`` int64 and the first / last ``min(max lag, n_shuffles)`` series rows
        (``lag_head`` / ``lag_tail``, uint16 ``n_rounds | won << 15``, ``[m][S]``) that ``rng_lags.LagSummary`` merges ranges with."""
        table, S, n_sh, spb, n_batches, ov, tally = self._setup(table, shuffle_begin, shuffle_end, shuffles_per_batch, overrides)
        lags, m, sums, head, tail = self._lag_arrays(lags, S, n_sh)
        self._check(self._lib.fk_tournament_run_lags(
            *self._lead(table, S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, ov, tally),
            _p(lags), len(lags), _p(sums), _p(head), _p(tail)))
        return {"tally": tally[:n_batches], "lag_sums": sums, "lag_head": head[:m], "lag_tail": tail[:m], "n_shuffles": n_sh}

    def tournament_matchups(self, table: np.ndarray, k: int, root_seed: int, shuffle_begin: int, shuffle_end: int, lags, strategy_ids,
                            max_players: int, shuffles_per_batch: int | None = None, target_score: int = 10_000, max_rounds: int = 200,
                            overrides: np.ndarray | None = None) -> dict:
        """``tournament_lags`` + the per-game records of the RNG diagnostics' matchup family (``fk_tournament_run_matchups``), in
        coordinate order: ``matchups = {"digest": uint64 [n], "seats": uint16 [n][k] (table indices in ascending-ID order),
        "rounds": uint16 [n]}``."""
        table, S, n_sh, spb, n_batches, ov, tally = self._setup(table, shuffle_begin, shuffle_end, shuffles_per_batch, overrides)
        lags, m, sums, head, tail = self._lag_arrays(lags, S, n_sh)
        ids = np.ascontiguousarray(strategy_ids, dtype=np.int32)
        if len(ids) != S or len(np.unique(ids)) != S:
            raise ValueError("strategy_ids must hold one unique ID per strategy of the table")
        n_games = n_sh * (S // k if k > 0 else 0)
        digest = np.zeros(max(n_games, 1), dtype=np.uint64)
        seats = np.zeros((max(n_games, 1), max(k, 1)), dtype=np.uint16)
        rounds = np.zeros(max(n_games, 1), dtype=np.uint16)
        self._check(self._lib.fk_tournament_run_matchups(
            *self._lead(table, S, k, root_seed, shuffle_begin, shuffle_end, spb, target_score, max_rounds, ov, tally),
            _p(lags), len(lags), _p(sums), _p(head), _p(tail), _p(ids), max_players, _p(digest), _p(seats), _p(rounds)))
        return {"tally": tally[:n_batches], "lag_sums": sums, "lag_head": head[:m], "lag_tail": tail[:m], "n_shuffles": n_sh,
                "matchups": {"digest": digest[:n_games], "seats": seats[:n_games], "rounds": rounds[:n_games]}}

    def matchup_reduce(self, records: dict, k: int, lags, cap: int | None) -> dict:
        """``fk_matchup_reduce`` over the records of a whole (root, k) in coordinate order: counts, histogram (``[min(lags) + 66]``
        groups per bin code) and the eligible groups of least priority — the first ``cap`` (``None`` / <= 0: all) plus every group
        tied with the last one kept — with their counts and per-lag sums ``[M][n_lags][6]`` (layout of ``rng_matchups.host_reduce``)."""
        lags_a = np.ascontiguousarray(list(lags), dtype=np.int32)
        digest = np.ascontiguousarray(records["digest"], dtype=np.uint64)
        k = int(k)
        seats = np.asarray(records["seats"], dtype=np.uint16)
        seats = np.ascontiguousarray(seats.reshape(-1, k) if k >= 1 else seats)  # (a k below 1 is the library's to refuse)
        rounds = np.ascontiguousarray(records["rounds"], dtype=np.uint16)
        n = len(digest)
        minimum = int(lags_a.min()) + 2 if len(lags_a) else 2
        cap_v = int(cap) if cap is not None and int(cap) > 0 else 0
        capacity = cap_v + 64 if cap_v else n // minimum + 1
        while True:
            counts = np.zeros(4, dtype=np.int64)
            hist = np.zeros(minimum + 64, dtype=np.uint64)
            out_d = np.zeros(max(capacity, 1), dtype=np.uint64)
            out_s = np.zeros((max(capacity, 1), max(k, 0)), dtype=np.uint16)
            out_c = np.zeros(max(capacity, 1), dtype=np.int64)
            out_x = np.zeros((max(capacity, 1), len(lags_a), 6), dtype=np.int64)
            rc = self._lib.fk_matchup_reduce(self._ctx, k, n, _p(digest), _p(seats), _p(rounds), _p(lags_a), len(lags_a), cap_v, capacity,
                                             _p(counts), _p(hist), _p(out_d), _p(out_s), _p(out_c), _p(out_x))
            if rc == FK_ERR_ARG and counts[3] > capacity:  # more priority ties than the slack: once more with room for all
                capacity = int(counts[3])
                continue
            self._check(rc)
            break
        M = int(counts[3])
        return {"k": int(k), "lags": tuple(int(v) for v in lags_a), "observations": int(counts[0]), "candidate_groups": int(counts[1]),
                "eligible_groups": int(counts[2]), "histogram": hist, "digest": out_d[:M], "seats": out_s[:M], "count": out_c[:M],
                "sums": out_x[:M]}

    def get_option(self, name: str) -> int:
        """``fk_get_option``: an option's value or a figure of the last call (``last_budget``, ``oom_replays``, the effective ``comm_timeout_ms``)."""
        value = C.c_int64(0)
        self._check(self._lib.fk_get_option(self._ctx, name.encode("utf-8"), C.byref(value)))
        return int(value.value)

    def hold_memory(self, leave_free: int) -> tuple[int, int]:
        """``fk_debug_hold_memory``: take device memory until about ``leave_free`` bytes are free (< 0: give it back); (free, total) after."""
        free, total = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.fk_debug_hold_memory(self._ctx, leave_free, C.byref(free), C.byref(total)))
        return int(free.value), int(total.value)

    def pinned_empty(self, n: int, dtype) -> np.ndarray:
        """``n`` elements of ``dtype`` in page-locked host memory (``fk_host_alloc``), freed when the array is collected — the
        ``rows_out`` buffer of rows mode.  Keep the engine alive while the array is."""
        import weakref

        dtype = np.dtype(dtype)
        nbytes = max(int(n) * dtype.itemsize, 1)
        ptr = C.c_void_p()
        self._check(self._lib.fk_host_alloc(self._ctx, nbytes, C.byref(ptr)))
        raw = (C.c_char * nbytes).from_address(ptr.value)
        arr = np.frombuffer(raw, dtype=dtype, count=int(n))
        lib, ctx, addr = self._lib, self._ctx, ptr.value
        weakref.finalize(raw, lambda: lib.fk_host_free(ctx, C.c_void_p(addr)) if ctx else None)
        return arr

    def hint_next(self, shuffle_begin: int, shuffle_end: int, need_state: bool = False) -> None:
        """The call after the next ``tournament`` call will play this shuffle range of the same table, k and root: its
        permutations and seat seeding are then prepared in the drain tail of the next call's game kernel."""
        self._check(self._lib.fk_tournament_hint_next(self._ctx, shuffle_begin, shuffle_end, 1 if need_state else 0))

    @staticmethod
    def _game_list(coords, table, seat_strategy, k) -> tuple:
        """What the explicit game-list entries take: the packed coordinates and table, the flat int32 seat strategies and n_games."""
        coords = np.ascontiguousarray(coords, dtype=COORD_DTYPE)
        table = np.ascontiguousarray(table, dtype=STRATEGY_DTYPE)
        ss = np.ascontiguousarray(seat_strategy, dtype=np.int32).reshape(-1)
        if ss.size != len(coords) * k:
            raise ValueError("seat_strategy must hold n_games * k entries")
        return coords, table, ss, len(coords)

    def play_games(self, coords: np.ndarray, table: np.ndarray, seat_strategy, k: int, target_score: int = 10_000,
                   max_rounds: int = 200) -> np.ndarray:
        coords, table, ss, n = self._game_list(coords, table, seat_strategy, k)
        rows = np.zeros(n, dtype=row_dtype(k))
        self._check(self._lib.fk_play_games(self._ctx, _p(coords), n, _p(table), len(table), _p(ss), k, target_score, max_rounds, _p(rows)))
        return rows

    def trace_games(self, coords: np.ndarray, table: np.ndarray, seat_strategy, k: int, target_score: int = 10_000,
                    max_rounds: int = 200) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``fk_trace_games``: the rows ``play_games`` returns for the same arguments, ``event_begin`` (int64 ``[n_games + 1]``) and
        the roll events of every game (``EVENT_DTYPE``; game g owns ``events[event_begin[g]:event_begin[g + 1]]``, in play order).
        A counting call sizes the event list, an exact-size call fills it."""
        coords, table, ss, n = self._game_list(coords, table, seat_strategy, k)
        rows = np.zeros(n, dtype=row_dtype(k))
        begin = np.zeros(n + 1, dtype=np.int64)
        lead = (self._ctx, _p(coords), n, _p(table), len(table), _p(ss), k, target_score, max_rounds, _p(rows), _p(begin))
        self._check(self._lib.fk_trace_games(*lead, None, 0))
        events = np.zeros(int(begin[-1]), dtype=EVENT_DTYPE)
        if len(events):
            self._check(self._lib.fk_trace_games(*lead, _p(events), len(events)))
        return rows, begin, events

    def census_games(self, coords: np.ndarray, table: np.ndarray, seat_strategy, k: int, target_score: int = 10_000,
                     max_rounds: int = 200, turn_bins: int = 256) -> dict:
        """``fk_census_games``: the roll census of an explicit game list — int64 ``roll_cells [6][61][7]``, ``strategy_dice [S][6][3]``,
        ``strategy_turns [S][3]``, ``turn_hist [S][turn_bins]`` (``include/farkle_hip.h``: ``fk_census``), equal to
        ``roll_census.RollCensus.from_events`` of what ``trace_games`` returns for the same arguments."""
        coords, table, ss, n = self._game_list(coords, table, seat_strategy, k)
        tables, census = _census_tables(len(table), turn_bins)
        self._check(self._lib.fk_census_games(self._ctx, _p(coords), n, _p(table), len(table), _p(ss), k, target_score, max_rounds,
                                              C.byref(census)))
        return tables

    def tournament_census(self, table: np.ndarray, k: int, root_seed: int, shuffle_begin: int, shuffle_end: int,
                          shuffles_per_batch: int | None = None, target_score: int = 10_000, max_rounds: int = 200,
                          overrides: np.ndarray | None = None, turn_bins: int = 256) -> dict:
        """``fk_tournament_run_census``: the roll census (the tables of ``census_games``) of the games ``tournament`` plays for the same
        range — the same permutations, seat streams and overrides."""
        table, S, n_sh, spb, n_batches, ov, _ = self._setup(table, shuffle_begin, shuffle_end, shuffles_per_batch, overrides)
        tables, census = _census_tables(S, turn_bins)
        self._check(self._lib.fk_tournament_run_census(self._ctx, _p(table), S, k, root_seed, shuffle_begin, max(shuffle_end, shuffle_begin),
                                                       spb, target_score, max_rounds, _p(ov), len(ov), C.byref(census)))
        return tables

    def h2h(self, seats: np.ndarray, root_seed: int, pair_id: int, order: int, target: int, max_attempts: int,
            chunk_games: int, target_score: int = 10_000, max_rounds: int = 200, overrides: np.ndarray | None = None,
            state=None) -> np.ndarray:
        seats = np.ascontiguousarray(seats, dtype=STRATEGY_DTYPE)
        if len(seats) != 2:
            raise ValueError("H2H blocks seat exactly two strategies")
        st = np.zeros(5, dtype=np.uint64) if state is None else np.ascontiguousarray(state, dtype=np.uint64).copy()
        ov = overrides if overrides is not None else np.zeros(0, dtype=OVERRIDE_DTYPE)
        ov = np.ascontiguousarray(ov, dtype=OVERRIDE_DTYPE)
        self._check(self._lib.fk_h2h_run(self._ctx, _p(seats), root_seed, pair_id, order, target, max_attempts, chunk_games, target_score,
                                         max_rounds, _p(ov), len(ov), _p(st)))
        return st

    def h2h_blocks(self, seats: np.ndarray, root_seed: int, pair_ids, orders, target, max_attempts, chunk_games=None,
                   target_score: int = 10_000, max_rounds: int = 200, overrides: np.ndarray | None = None,
                   states: np.ndarray | None = None) -> np.ndarray:
        """Many (pair, order) blocks of one root advanced in shared kernel launches (``fk_h2h_run_blocks``): ``seats[b]`` =
        the two seated strategies of block b; ``target`` / ``max_attempts`` scalars or per-block arrays; ``states`` the
        blocks' progress so far (default: fresh).  Returns uint64 ``[n_blocks][5]`` = attempted, completed, safety,
        wins_seat1, wins_seat2 — each row equals the serial ``h2h`` result of that block."""
        seats = np.ascontiguousarray(seats, dtype=STRATEGY_DTYPE).reshape(-1, 2)
        n = len(seats)
        blocks = np.zeros(n, dtype=H2H_BLOCK_DTYPE)
        blocks["seats"] = seats
        blocks["pair_id"] = np.asarray(pair_ids, dtype=np.uint64).reshape(-1)
        blocks["order"] = np.asarray(orders, dtype=np.uint32).reshape(-1)
        blocks["target"] = np.asarray(target, dtype=np.uint64)
        blocks["max_attempts"] = np.asarray(max_attempts, dtype=np.uint64)
        if states is not None:
            blocks["state"] = np.asarray(states, dtype=np.uint64).reshape(n, 5)
        chunk = int(blocks["max_attempts"].max()) if chunk_games is None and n else int(chunk_games or 0)
        ov = overrides if overrides is not None else np.zeros(0, dtype=OVERRIDE_DTYPE)
        ov = np.ascontiguousarray(ov, dtype=OVERRIDE_DTYPE)
        self._check(self._lib.fk_h2h_run_blocks(self._ctx, _p(blocks), n, root_seed, chunk, target_score, max_rounds, _p(ov), len(ov)))
        return blocks["state"].copy()

    def h2h_round_robin(self, table: np.ndarray, root_seed: int, target: int, max_attempts: int, pair_begin: int = 0,
                        pair_end: int | None = None, target_score: int = 10_000, max_rounds: int = 200,
                        summary: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Head-to-head round robin (``fk_h2h_round_robin``): pairs ``[pair_begin, pair_end)`` of ``table`` — sorted by strategy id, pairs
        numbered as ``itertools.combinations(range(n), 2)`` — both seat orders, every block fresh and played to its terminal status.
        Returns ``(states, summary)``: uint32 ``[pairs, 2, 5]`` = attempted, completed, safety, wins_seat1, wins_seat2 per (pair, order),
        and int64 ``[n, 8]`` (``round_robin.SUMMARY_COLS``).  A ``summary`` handed in is added to in place (pair ranges and roots
        accumulate) and returned."""
        table = np.ascontiguousarray(table, dtype=STRATEGY_DTYPE).reshape(-1)
        n = len(table)
        end = n * (n - 1) // 2 if pair_end is None else int(pair_end)
        begin = int(pair_begin)
        if summary is None:
            summary = np.zeros((n, 8), dtype=np.int64)
        elif not (isinstance(summary, np.ndarray) and summary.dtype == np.int64 and summary.shape == (n, 8) and summary.flags.c_contiguous):
            raise ValueError(f"summary must be a C-contiguous int64 array of shape {(n, 8)}")
        if min(begin, end, int(target), int(max_attempts), int(root_seed)) < 0:
            raise ValueError("pair range, target, max_attempts and root_seed must not be negative")
        states = np.zeros((max(end - begin, 0), 2, 5), dtype=np.uint32)
        self._check(self._lib.fk_h2h_round_robin(self._ctx, _p(table), n, root_seed, begin, end, target, max_attempts, target_score, max_rounds,
                                                 _p(states), _p(summary)))
        return states, summary

    def _rr_range(self, table, pair_begin, pair_end, family_pair_count) -> tuple:
        table = np.ascontiguousarray(table, dtype=STRATEGY_DTYPE).reshape(-1)
        n = len(table)
        end = n * (n - 1) // 2 if pair_end is None else int(pair_end)
        begin = int(pair_begin)
        family = n * (n - 1) // 2 if family_pair_count is None else int(family_pair_count)
        if min(begin, end, family) < 0:
            raise ValueError("pair range and family_pair_count must not be negative")
        return table, n, begin, end, family

    def h2h_round_robin_resident(self, table: np.ndarray, root_seed: int, target: int, max_attempts: int, pair_begin: int = 0,
                                 pair_end: int | None = None, target_score: int = 10_000, max_rounds: int = 200,
                                 summary: np.ndarray | None = None, family_pair_count: int | None = None) -> np.ndarray:
        """``fk_h2h_round_robin_resident``: ``h2h_round_robin`` whose block states stay on the device and are added to the context's pair
        counts (one call per root; the first fixes table, range and ``family_pair_count`` — default the table's pair count).  Returns the
        summary, as ``h2h_round_robin`` does."""
        table, n, begin, end, family = self._rr_range(table, pair_begin, pair_end, family_pair_count)
        if summary is None:
            summary = np.zeros((n, 8), dtype=np.int64)
        elif not (isinstance(summary, np.ndarray) and summary.dtype == np.int64 and summary.shape == (n, 8) and summary.flags.c_contiguous):
            raise ValueError(f"summary must be a C-contiguous int64 array of shape {(n, 8)}")
        if min(int(target), int(max_attempts), int(root_seed)) < 0:
            raise ValueError("target, max_attempts and root_seed must not be negative")
        self._check(self._lib.fk_h2h_round_robin_resident(self._ctx, _p(table), n, root_seed, begin, end, target, max_attempts, target_score,
                                                          max_rounds, _p(summary), family))
        self._rr_n = n
        return summary

    def rr_counts_add(self, table: np.ndarray, states: np.ndarray, target: int, max_attempts: int, pair_begin: int = 0,
                      pair_end: int | None = None, family_pair_count: int | None = None, root_seed: int | None = None) -> None:
        """``fk_rr_counts_add``: one root's host-held block states ``[pairs, 2, 5]`` (as ``h2h_round_robin`` returned them for this
        ``target`` / ``max_attempts``) into the context's pair counts.  With ``root_seed`` it is ``fk_rr_counts_add_root``: under option
        ``"rr_keep_roots"`` the states are also kept on the device, for ``rr_root_diagnostics``."""
        table, n, begin, end, family = self._rr_range(table, pair_begin, pair_end, family_pair_count)
        st = np.asarray(states)
        if st.shape != (max(end - begin, 0), 2, 5) or st.dtype.kind not in "iu" or (st.size and (int(st.min()) < 0 or int(st.max()) > 0xFFFFFFFF)):
            raise ValueError(f"states must be unsigned 32-bit counts of shape {(max(end - begin, 0), 2, 5)}")
        st = np.ascontiguousarray(st, dtype=np.uint32)
        if min(int(target), int(max_attempts)) < 0:
            raise ValueError("target and max_attempts must not be negative")
        args = (self._ctx, _p(table), n, begin, end, target, max_attempts, _p(st), family)
        if root_seed is None:
            self._check(self._lib.fk_rr_counts_add(*args))
        else:
            if not 0 <= int(root_seed) < 1 << 64:
                raise ValueError("root_seed must fit 64 unsigned bits")
            self._check(self._lib.fk_rr_counts_add_root(*args, int(root_seed)))
        self._rr_n = n

    def rr_counts_reset(self) -> None:
        """``fk_rr_counts_reset``: forget the resident pair counts."""
        self._check(self._lib.fk_rr_counts_reset(self._ctx))
        self._rr_n = 0

    def _rr_params(self, family_alpha, practical_delta, delta_equivalence, min_candidate_completion_rate, family_pair_count) -> _RrInferenceParams:
        """``fk_rr_inference_params``; the two critical values are evaluated here, once, with scipy (``norm.isf``)."""
        from scipy.stats import norm

        n = self._rr_n
        family = n * (n - 1) // 2 if family_pair_count is None else int(family_pair_count)
        if family < 0 or family >= 1 << 64:
            raise ValueError("family_pair_count must fit 64 unsigned bits")
        alpha = float(family_alpha)
        ok = 0.0 < alpha < 1.0 and family > 0  # (the entry refuses the others with its own message; isf of them is undefined)
        return _RrInferenceParams(alpha, float(practical_delta), float("nan") if delta_equivalence is None else float(delta_equivalence),
                                  float(min_candidate_completion_rate), float(norm.isf(alpha / 2.0)) if ok else 1.0,
                                  float(norm.isf(alpha / family / 2.0)) if ok else 1.0, family)

    def rr_inference(self, family_alpha: float = 0.02, practical_delta: float = 0.03, delta_equivalence: float | None = None,
                     min_candidate_completion_rate: float = 0.99, family_pair_count: int | None = None,
                     rows: tuple[int, int] | None = None, want_strategies: bool = True) -> dict:
        """``fk_rr_inference`` over the resident pair counts (of an ``n``-row table): ``{"class_counts": int64 [7], "strategies": int64
        [n, 12] or None, "rows": RR_PAIR_ROW_DTYPE [row_end - row_begin] or None}``.  ``rows`` is a pair-id range ``(begin, end)``.  The two
        critical values are evaluated here, once, with scipy (``norm.isf``), as the reference's ``_score_difference_interval_fallback`` does."""
        n = self._rr_n  # the table size fixed with the resident counts: it sizes the per-strategy output
        par = self._rr_params(family_alpha, practical_delta, delta_equivalence, min_candidate_completion_rate, family_pair_count)
        out_rows, begin, end = None, 0, 0
        if rows is not None:
            begin, end = int(rows[0]), int(rows[1])
            if begin < 0 or end < 0:
                raise ValueError("the row range must not be negative")
            out_rows = np.zeros(max(end - begin, 0), dtype=RR_PAIR_ROW_DTYPE)
        class_counts = np.zeros(RR_CLASSES, dtype=np.int64)
        strategies = np.zeros((n, RR_STRATEGY_COLS), dtype=np.int64) if want_strategies else None
        self._check(self._lib.fk_rr_inference(self._ctx, C.byref(par), _p(out_rows), begin, end, _p(class_counts), _p(strategies)))
        return {"class_counts": class_counts, "strategies": strategies, "rows": out_rows}

    def rr_root_diagnostics(self, family_alpha: float = 0.02, practical_delta: float = 0.03, delta_equivalence: float | None = None,
                            min_candidate_completion_rate: float = 0.99, family_pair_count: int | None = None,
                            rows: tuple[int, int] | None = None, want_agreement: bool = True) -> dict:
        """``fk_rr_root_diagnostics`` over the resident pair counts and the root states kept with them (option ``"rr_keep_roots"``):
        ``{"roots": uint64 [n_roots] ascending, "rows": RR_ROOT_ROW_DTYPE [n_roots, k] or None, "agreement": RR_AGREEMENT_ROW_DTYPE [k] or
        None, "summary": int64 [12], "max_abs_discrepancy": float}``, ``k`` the pairs of the pair-id range ``rows``.  The parameters are
        ``rr_inference``'s."""
        par = self._rr_params(family_alpha, practical_delta, delta_equivalence, min_candidate_completion_rate, family_pair_count)
        out_rows = agreement = None
        begin = end = 0
        if rows is not None:
            begin, end = int(rows[0]), int(rows[1])
            if begin < 0 or end < 0:
                raise ValueError("the row range must not be negative")
            out_rows = np.zeros((RR_MAX_ROOTS, max(end - begin, 0)), dtype=RR_ROOT_ROW_DTYPE)
            agreement = np.zeros(max(end - begin, 0), dtype=RR_AGREEMENT_ROW_DTYPE) if want_agreement else None
        seeds = np.zeros(RR_MAX_ROOTS, dtype=np.uint64)
        n_roots = C.c_int32(0)
        summary = np.zeros(RR_AGREE_COLS, dtype=np.int64)
        largest = C.c_double(float("nan"))
        self._check(self._lib.fk_rr_root_diagnostics(self._ctx, C.byref(par), _p(seeds), C.byref(n_roots), _p(out_rows), begin, end,
                                                     _p(agreement), _p(summary), C.byref(largest)))
        if out_rows is not None:  # the entry wrote [n_roots][k] at the front of the buffer
            out_rows = out_rows.reshape(-1)[: n_roots.value * out_rows.shape[1]].reshape(n_roots.value, out_rows.shape[1])
        return {"roots": seeds[: n_roots.value].copy(), "rows": out_rows, "agreement": agreement, "summary": summary,
                "max_abs_discrepancy": float(largest.value)}

    @staticmethod
    def _dominance_outputs(n: int, rank, want_adjacency: bool) -> tuple:
        if rank is not None:
            rank = np.asarray(rank)
            if rank.shape != (n,) or rank.dtype.kind not in "iu" or (rank.size and (int(rank.min()) < 0 or int(rank.max()) > 0xFFFFFFFF)):
                raise ValueError(f"rank must hold {n} unsigned 32-bit positions")
            rank = np.ascontiguousarray(rank, dtype=np.uint32)
        nodes = np.zeros(max(n, 0), dtype=DOM_NODE_DTYPE)
        extremes = np.zeros((2, max(n, 0)), dtype=DOM_EXTREME_DTYPE)
        adjacency = np.zeros((2, max(n, 0), (max(n, 0) + 63) // 64), dtype=np.uint64) if want_adjacency else None
        return rank, nodes, extremes, adjacency

    def dominance_graph(self, n: int, decision_class, sim_d_low, sim_d_high, balanced_rate, practical_delta: float = 0.03, rank=None,
                        want_adjacency: bool = True) -> dict:
        """``fk_dominance_graph``: the practical (index 0) and statistical (index 1) dominance graphs of an ``n``-row table from its pairs'
        decision classes, simultaneous d bounds and balanced rates, arrays of ``n (n - 1) / 2`` in pair-id order.  ``rank[row]`` orders the
        strategies where two internal edges are equally strong (None: table order).  Returns ``{"nodes": DOM_NODE_DTYPE [n], "extremes":
        DOM_EXTREME_DTYPE [2, n], "adjacency": uint64 [2, n, ceil(n / 64)] or None}``."""
        n = int(n)
        n_pairs = max(n * (n - 1) // 2, 0)
        cls = np.ascontiguousarray(decision_class, dtype=np.uint8).reshape(-1)
        arrays = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (sim_d_low, sim_d_high, balanced_rate)]
        if 2 <= n <= DOM_MAX_N and any(len(a) != n_pairs for a in (cls, *arrays)):  # (the entry refuses the other sizes before it reads an array)
            raise ValueError(f"a table of {n} strategies has {n_pairs} pairs")
        rank, nodes, extremes, adjacency = self._dominance_outputs(n, rank, want_adjacency)
        self._check(self._lib.fk_dominance_graph(self._ctx, n, _p(cls), _p(arrays[0]), _p(arrays[1]), _p(arrays[2]), practical_delta,
                                                 _p(rank), _p(nodes), _p(extremes), _p(adjacency)))
        return {"nodes": nodes, "extremes": extremes, "adjacency": adjacency}

    def rr_dominance(self, family_alpha: float = 0.02, practical_delta: float = 0.03, delta_equivalence: float | None = None,
                     min_candidate_completion_rate: float = 0.99, family_pair_count: int | None = None, rank=None,
                     want_adjacency: bool = True) -> dict:
        """``fk_rr_dominance``: ``rr_inference`` over the resident pair counts, its classes, bounds and rates fed to the graph kernels of
        ``dominance_graph`` on the device.  The resident range must be the whole table.  Returns ``dominance_graph``'s dictionary and
        ``"class_counts"``."""
        n = self._rr_n
        par = self._rr_params(family_alpha, practical_delta, delta_equivalence, min_candidate_completion_rate, family_pair_count)
        rank, nodes, extremes, adjacency = self._dominance_outputs(n, rank, want_adjacency)
        class_counts = np.zeros(RR_CLASSES, dtype=np.int64)
        self._check(self._lib.fk_rr_dominance(self._ctx, C.byref(par), _p(rank), _p(nodes), _p(extremes), _p(adjacency), _p(class_counts)))
        return {"nodes": nodes, "extremes": extremes, "adjacency": adjacency, "class_counts": class_counts}

    @staticmethod
    def _int32_array(values, what: str) -> np.ndarray:
        a = np.asarray(values)
        if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (int(a.min()) < -(1 << 31) or int(a.max()) >= 1 << 31)):
            raise ValueError(f"{what} must be a one-dimensional array of 32-bit integers")
        return np.ascontiguousarray(a, dtype=np.int32)

    def _agreement_ranks(self, n: int, win_rate_rank, trueskill_rank, sized: bool = True) -> tuple:
        win, ts = self._int32_array(win_rate_rank, "win_rate_rank"), self._int32_array(trueskill_rank, "trueskill_rank")
        if sized and not len(win) == len(ts) == n:  # (the entry refuses the other sizes before it reads an array)
            raise ValueError(f"the two rank arrays must name the {n} rows of the table")
        return win, ts

    def agreement_pairs(self, n: int, decision_class, win_rate_rank, trueskill_rank, want_codes: bool = True) -> dict:
        """``fk_agreement_pairs``: every pair's code byte (bits 0-1 ``h2h_direction``, 2-3 ``win_rate_preference``, 4-5
        ``trueskill_preference``; 0 none, 1 a, 2 b) and the eleven counts, from the pairs' decision classes in pair-id order and the two
        ranks of every table row (``AGREE_NO_RANK`` = 0 is null).  Returns ``{"codes": uint8 [pairs] or None, "counts": int64 [11]}``."""
        n = int(n)
        n_pairs = max(n * (n - 1) // 2, 0)
        cls = np.ascontiguousarray(decision_class, dtype=np.uint8).reshape(-1)
        sized = 2 <= n and n_pairs < 1 << 31
        win, ts = self._agreement_ranks(n, win_rate_rank, trueskill_rank, sized)
        if sized and len(cls) != n_pairs:
            raise ValueError(f"a table of {n} strategies has {n_pairs} pairs")
        codes = np.zeros(n_pairs if sized else 0, dtype=np.uint8) if want_codes else None
        counts = np.zeros(AGREE_COUNTS, dtype=np.int64)
        self._check(self._lib.fk_agreement_pairs(self._ctx, n, _p(cls), _p(win), _p(ts), _p(codes), _p(counts)))
        return {"codes": codes, "counts": counts}

    def rr_agreement(self, win_rate_rank, trueskill_rank, family_alpha: float = 0.02, practical_delta: float = 0.03,
                     delta_equivalence: float | None = None, min_candidate_completion_rate: float = 0.99, family_pair_count: int | None = None,
                     want_codes: bool = True) -> dict:
        """``fk_rr_agreement``: ``rr_inference`` over the resident pair counts, its classes fed to the pair kernel of ``agreement_pairs``
        on the device.  The resident range must be the whole table.  Returns ``agreement_pairs``' dictionary and ``"class_counts"``."""
        n = self._rr_n
        par = self._rr_params(family_alpha, practical_delta, delta_equivalence, min_candidate_completion_rate, family_pair_count)
        win, ts = self._agreement_ranks(n, win_rate_rank, trueskill_rank, n >= 2)  # (n = 0: no resident counts, which the entry refuses)
        codes = np.zeros(max(n * (n - 1) // 2, 0), dtype=np.uint8) if want_codes else None
        counts = np.zeros(AGREE_COUNTS, dtype=np.int64)
        class_counts = np.zeros(RR_CLASSES, dtype=np.int64)
        self._check(self._lib.fk_rr_agreement(self._ctx, C.byref(par), _p(win), _p(ts), _p(codes), _p(counts), _p(class_counts)))
        return {"codes": codes, "counts": counts, "class_counts": class_counts}

    def rank_concordance(self, x, y) -> np.ndarray:
        """``fk_rank_concordance``: Kendall's pair counts of the items with keys ``x``, ``y`` (each at least 1) over all ``i < j``: int64
        ``[5]`` = concordant, discordant, tied in ``x`` only, tied in ``y`` only, tied in both."""
        x, y = self._int32_array(x, "x"), self._int32_array(y, "y")
        if len(x) != len(y):
            raise ValueError("x and y must have one key per item each")
        counts = np.zeros(CONCORDANCE_COUNTS, dtype=np.int64)
        self._check(self._lib.fk_rank_concordance(self._ctx, min(len(x), (1 << 31) - 1), _p(x), _p(y), _p(counts)))
        return counts

    def score_power_scan(self, cells, alpha: float) -> np.ndarray:
        """``fk_score_power_scan``: exact power of the two-sided score test at level ``alpha`` for every cell of ``cells``
        (``POWER_CELL_DTYPE``: ``n`` completed games per order, ``q_ab``, ``q_ba``; ``h2h_power.make_cells`` builds them), float64
        ``[cells]`` in the cells' order.  The critical value is evaluated here, once, with scipy (``norm.isf(alpha / 2)``)."""
        from scipy.stats import norm

        cells = np.ascontiguousarray(cells, dtype=POWER_CELL_DTYPE).reshape(-1)
        alpha = float(alpha)
        if not 0.0 < alpha < 1.0:
            raise ValueError(f"alpha must be in (0, 1), got {alpha}")
        power = np.zeros(len(cells), dtype=np.float64)
        self._check(self._lib.fk_score_power_scan(self._ctx, _p(cells), len(cells), float(norm.isf(alpha / 2.0)), _p(power)))
        return power

    # -- multi-GPU: the one exchange of the path, RCCL through the C-ABI ---------------------
    def comm_unique_id(self) -> bytes:
        """Rank 0: a fresh RCCL communicator id (128 bytes) to ship to every rank."""
        buf = C.create_string_buffer(COMM_ID_BYTES)
        rc = self._lib.fk_comm_unique_id(buf)
        if rc != 0:
            raise FarkleHipError(rc, "fk_comm_unique_id failed: librccl.so.1 could not be loaded or ncclGetUniqueId failed")
        return buf.raw

    def comm_init(self, comm_id: bytes, rank: int, world_size: int) -> None:
        """Collective: every rank joins the communicator on its own GPU."""
        if len(comm_id) != COMM_ID_BYTES:
            raise ValueError("communicator id must be 128 bytes")
        self._check(self._lib.fk_comm_init(self._ctx, C.create_string_buffer(comm_id, COMM_ID_BYTES), rank, world_size))
        self.comm_world = world_size
        self.comm_rank = rank

    def reduce_tally(self, tally: np.ndarray, root: int = 0) -> np.ndarray:
        """Collective: int64 SUM over the communicator; the total on ``root`` (the rank's own tally elsewhere)."""
        t = np.ascontiguousarray(tally, dtype=np.int64).copy()
        self._check(self._lib.fk_reduce_tally(self._ctx, _p(t), t.size, root))
        return t

    def reduce_resident_tally(self, shape, root: int = 0) -> np.ndarray | None:
        """Collective: the device-resident tally accumulator (option ``resident_tally``) summed over the communicator on the
        device; the total on ``root`` (None elsewhere).  Clears the accumulator."""
        out = np.zeros(shape, dtype=np.int64)
        self._check(self._lib.fk_tally_resident_reduce(self._ctx, _p(out), out.size, root))
        return out if (self.comm_world == 1 or self.comm_rank == root) else None

    def comm_ranks(self) -> int:
        """Ranks of the engine's RCCL communicator as RCCL counts them (1 without one)."""
        return int(self._lib.fk_comm_ranks(self._ctx))

    def comm_destroy(self) -> None:
        self._check(self._lib.fk_comm_destroy(self._ctx))
        self.comm_world = 1

    def coordinate_seeds(self, coords: np.ndarray, want32: bool = True, want64: bool = False):
        """SeedSequence fingerprints of whole coordinates (``coordinate_seed``, utils/random.py:190-232)."""
        coords = np.ascontiguousarray(coords, dtype=COORD_DTYPE)
        n = len(coords)
        s32 = np.zeros(n, dtype=np.uint32) if want32 else None
        s64 = np.zeros(n, dtype=np.uint64) if want64 else None
        self._check(self._lib.fk_coordinate_seeds(self._ctx, n, _p(coords), _p(s32), _p(s64)))
        return s32, s64

    def game_seeds(self, purpose: int, root_seed: int, k: int, shuffle_begin: int, shuffle_end: int, games_per_shuffle: int) -> np.ndarray:
        """uint32 ``coordinate_seed`` fingerprints ``[n_shuffles][games_per_shuffle]`` of (purpose, root, k, shuffle, game_index)."""
        n_sh = max(int(shuffle_end) - int(shuffle_begin), 0)
        out = np.zeros((n_sh, int(games_per_shuffle)), dtype=np.uint32)
        self._check(self._lib.fk_game_seeds(self._ctx, int(purpose), root_seed, k, shuffle_begin, n_sh, int(games_per_shuffle), _p(out)))
        return out

    # -- single-op probes ------------------------------------------------------------------
    def debug_score(self, faces: np.ndarray, lens, pre, strategies: np.ndarray) -> np.ndarray:
        faces = np.ascontiguousarray(faces, dtype=np.uint8).reshape(-1, 6)
        n = len(faces)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        pre = np.ascontiguousarray(pre, dtype=np.int32)
        strategies = np.ascontiguousarray(strategies, dtype=STRATEGY_DTYPE)
        out = np.zeros((n, 5), dtype=np.int32)
        self._check(self._lib.fk_debug_score(self._ctx, n, _p(faces), _p(lens), _p(pre), _p(strategies), _p(out)))
        return out

    def debug_should_continue(self, args: np.ndarray, strategies: np.ndarray) -> np.ndarray:
        args = np.ascontiguousarray(args, dtype=np.int32).reshape(-1, 6)
        strategies = np.ascontiguousarray(strategies, dtype=STRATEGY_DTYPE)
        out = np.zeros(len(args), dtype=np.int32)
        self._check(self._lib.fk_debug_should_continue(self._ctx, len(args), _p(args), _p(strategies), _p(out)))
        return out

    def debug_dice(self, coords: np.ndarray, sizes, want_raw: bool = True):
        coords = np.ascontiguousarray(coords, dtype=COORD_DTYPE)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        n = len(coords)
        faces = np.zeros((n, int(sizes.sum())), dtype=np.uint8)
        raw = np.zeros((n, 4), dtype=np.uint64) if want_raw else None
        self._check(self._lib.fk_debug_dice(self._ctx, n, _p(coords), len(sizes), _p(sizes), _p(faces), _p(raw)))
        return faces, raw

    def debug_bounded_draws(self, coords: np.ndarray, bound: int, n_draws: int) -> np.ndarray:
        """``fk_debug_bounded_draws``: uint32 ``[n][n_draws]`` = ``Generator(PCG64DXSM(coords[i])).integers(0, bound, size=n_draws)`` by
        the bootstrap's own device draw function (1 <= bound <= 2**32 - 1)."""
        coords = np.ascontiguousarray(coords, dtype=COORD_DTYPE)
        out = np.zeros((len(coords), int(n_draws)), dtype=np.uint32)
        self._check(self._lib.fk_debug_bounded_draws(self._ctx, len(coords), _p(coords), int(bound), int(n_draws), _p(out)))
        return out

    def debug_perm_from_draws(self, S: int, draws: np.ndarray, path: int, out: np.ndarray | None = None, n_sh: int | None = None) -> np.ndarray:
        """``fk_debug_perm_from_draws``: int32 ``[n_sh][S]``, the Fisher-Yates result of every row of uint16 ``draws [n_sh][S - 1]``
        (draw ``n`` is the ``j`` of step ``S - 1 - n``, so ``draws[:, n] <= S - 1 - n``) by the swap-chain kernel (``path`` 1) or the
        chain-free kernel (``path`` 2).  ``out``: the caller's result array (a refused call leaves it as it was); ``n_sh``: the shuffle
        count handed to the entry when it is not ``len(draws)`` (refusal tests)."""
        draws = np.ascontiguousarray(draws, dtype=np.uint16)
        if n_sh is None:
            n_sh = len(draws) if draws.ndim == 2 else draws.size // max(int(S) - 1, 1)
        if out is None:
            out = np.zeros((max(int(n_sh), 0), max(int(S), 0)), dtype=np.int32)
        assert out.dtype == np.int32 and out.flags.c_contiguous
        assert n_sh < 1 or S < 1 or (out.size == n_sh * S and draws.size == n_sh * (S - 1)), "draws [n_sh][S - 1] and out [n_sh][S]"
        self._check(self._lib.fk_debug_perm_from_draws(self._ctx, int(S), int(n_sh), _p(draws), int(path), _p(out)))
        return out

    def performance_bootstrap(self, root_seed: int, ks, wins, exposures, replicate_begin: int, replicate_end: int, top_n: int,
                              delta: float, controls=(), want_scores: bool = True, contrast_sum: np.ndarray | None = None,
                              contrast_square_sum: np.ndarray | None = None) -> dict:
        """``fk_performance_bootstrap``: the joint deterministic-batch bootstrap of replicates ``[replicate_begin, replicate_end)``.
        ``wins[i]`` / ``exposures[i]``: int64 ``[B_i][S]`` of player count ``ks[i]``, eligible batches only, columns in ascending
        strategy id; ``controls``: column indices.  Returns ``scores`` (float64 ``[R][S]`` or None), int64 ``rank_sum``,
        ``rank_square_sum``, ``top_counts``, ``shortlist_counts`` of THIS range and float64 ``contrast_sum`` /
        ``contrast_square_sum`` ``[C][S]`` continued from the arrays passed in (zeros when omitted)."""
        ks = [int(v) for v in ks]
        if len(ks) != len(wins) or len(ks) != len(exposures) or not ks:
            raise ValueError("one wins and one exposures matrix per player count")
        W = [np.ascontiguousarray(m, dtype=np.int64) for m in wins]
        E = [np.ascontiguousarray(m, dtype=np.int64) for m in exposures]
        S = int(W[0].shape[1]) if W[0].ndim == 2 else -1
        for w, e in zip(W, E):
            if w.ndim != 2 or w.shape != e.shape or w.shape[1] != S:
                raise ValueError("every matrix is [batches][S] with one S")
        n_k = len(ks)
        R = max(int(replicate_end) - int(replicate_begin), 0)
        ctrl = np.ascontiguousarray(list(controls), dtype=np.int32)
        n_ctrl = len(ctrl)
        scores = np.zeros((R, S), dtype=np.float64) if want_scores else None
        counters = [np.zeros(S, dtype=np.int64) for _ in range(4)]
        csum = np.zeros((n_ctrl, S), np.float64) if contrast_sum is None else np.array(contrast_sum, dtype=np.float64, order="C").reshape(n_ctrl, S)
        csq = np.zeros((n_ctrl, S), np.float64) if contrast_square_sum is None else np.array(contrast_square_sum, dtype=np.float64, order="C").reshape(n_ctrl, S)
        k_arr = np.asarray(ks, dtype=np.int32)
        b_arr = np.asarray([len(m) for m in W], dtype=np.int64)
        w_ptr = (C.c_void_p * n_k)(*[m.ctypes.data for m in W])
        e_ptr = (C.c_void_p * n_k)(*[m.ctypes.data for m in E])
        self._check(self._lib.fk_performance_bootstrap(
            self._ctx, int(root_seed), n_k, _p(k_arr), _p(b_arr), w_ptr, e_ptr, S, int(replicate_begin), int(replicate_end), int(top_n),
            float(delta), n_ctrl, _p(ctrl) if n_ctrl else None, _p(scores), *[_p(a) for a in counters], _p(csum) if n_ctrl else None,
            _p(csq) if n_ctrl else None))
        return {"scores": scores, "rank_sum": counters[0], "rank_square_sum": counters[1], "top_counts": counters[2],
                "shortlist_counts": counters[3], "contrast_sum": csum, "contrast_square_sum": csq}

    def root_stability_bootstrap(self, roots, ks, wins, exposures, weights, replicate_begin: int, replicate_end: int, top_n: int,
                                 observed=None, expected=None, observed_across=None, expected_across=None,
                                 want_membership: bool = False) -> dict:
        """``fk_root_stability_bootstrap``: the two-root stability stage's bootstrap families for replicates ``[replicate_begin,
        replicate_end)``.  ``wins[c]`` / ``exposures[c]``: int64 ``[B_c][S]`` of cell ``c`` in (root, k) order — ``roots[0]``'s player
        counts ``ks``, then ``roots[1]``'s — eligible batches only; ``weights``: one per player count.  ``observed`` / ``expected``
        ``[n_k][S]`` and ``observed_across`` / ``expected_across`` ``[S]`` come as a group or not at all (top-N family only).
        Returns int64 ``top_counts`` ``[2][S]``, float64 ``maxima`` ``[R]`` (None without the group) and uint8 ``membership``
        ``[R][2][S]`` (None unless asked for)."""
        ks = [int(v) for v in ks]
        n_k = len(ks)
        if not n_k or len(wins) != 2 * n_k or len(exposures) != 2 * n_k or len(list(weights)) != n_k or len(list(roots)) != 2:
            raise ValueError("two roots, one weight per player count and one wins / exposures matrix per (root, player count) cell")
        W = [np.ascontiguousarray(m, dtype=np.int64) for m in wins]
        E = [np.ascontiguousarray(m, dtype=np.int64) for m in exposures]
        S = int(W[0].shape[1]) if W[0].ndim == 2 else -1
        for w, e in zip(W, E):
            if w.ndim != 2 or w.shape != e.shape or w.shape[1] != S:
                raise ValueError("every matrix is [batches][S] with one S")
        group = [observed, expected, observed_across, expected_across]
        if sum(v is not None for v in group) not in (0, 4):
            raise ValueError("observed / expected by k and across k come as a group of four")
        joint = observed is not None
        if joint:
            group = [np.ascontiguousarray(v, dtype=np.float64) for v in group]
            if group[0].shape != (n_k, S) or group[1].shape != (n_k, S) or group[2].shape != (S,) or group[3].shape != (S,):
                raise ValueError("observed / expected are [n_k][S], observed_across / expected_across [S]")
        R = max(int(replicate_end) - int(replicate_begin), 0)
        root_arr = np.asarray([int(r) for r in roots], dtype=np.uint64)
        k_arr = np.asarray(ks, dtype=np.int32)
        b_arr = np.asarray([len(m) for m in W], dtype=np.int64)
        w_arr = np.asarray([float(w) for w in weights], dtype=np.float64)
        w_ptr = (C.c_void_p * (2 * n_k))(*[m.ctypes.data for m in W])
        e_ptr = (C.c_void_p * (2 * n_k))(*[m.ctypes.data for m in E])
        top_counts = np.zeros((2, S), dtype=np.int64)
        maxima = np.zeros(R, dtype=np.float64) if joint else None
        membership = np.zeros((R, 2, S), dtype=np.uint8) if want_membership else None
        self._check(self._lib.fk_root_stability_bootstrap(
            self._ctx, _p(root_arr), n_k, _p(k_arr), _p(b_arr), w_ptr, e_ptr, S, _p(w_arr), int(replicate_begin), int(replicate_end), int(top_n),
            *[_p(v) if joint else None for v in group], _p(top_counts), _p(maxima), _p(membership)))
        return {"top_counts": top_counts, "maxima": maxima, "membership": membership}

    def performance_by_k(self, k: int, wins, exposures, completed, safety, B: int | None = None, S: int | None = None) -> dict:
        """``fk_performance_by_k``: the per-k point estimates' sums over ALL batches of one player count.  Four int64 ``[B][S]``
        matrices (rows in ascending batch id, columns in ascending strategy id; cells without an exposure allowed).  Returns int64
        ``[S]`` ``wins``, ``exposures``, ``completed``, ``safety``, ``losses``, ``positive_batches`` and float64 ``[S]`` ``rate_sum``,
        ``ssd`` (NumPy's summation order, ``performance.host_by_k`` bit for bit).  ``B`` / ``S``: the shape handed to the entry when
        it is not the matrices' (refusal tests)."""
        mats = [np.ascontiguousarray(m, dtype=np.int64) for m in (wins, exposures, completed, safety)]
        if mats[0].ndim != 2 or any(m.shape != mats[0].shape for m in mats):
            raise ValueError("wins, exposures, completed and safety are [batches][S] matrices of one shape")
        B = mats[0].shape[0] if B is None else int(B)
        S = mats[0].shape[1] if S is None else int(S)
        names = ("wins", "exposures", "completed", "safety", "losses", "positive_batches")
        out = {name: np.zeros(max(S, 0), dtype=np.int64) for name in names}
        out["rate_sum"], out["ssd"] = np.zeros(max(S, 0), dtype=np.float64), np.zeros(max(S, 0), dtype=np.float64)
        self._check(self._lib.fk_performance_by_k(self._ctx, int(k), B, S, _p(mats[0]), _p(mats[1]), _p(mats[2]), _p(mats[3]), _p(out["wins"]),
                                                  _p(out["exposures"]), _p(out["completed"]), _p(out["safety"]), _p(out["losses"]),
                                                  _p(out["positive_batches"]), _p(out["rate_sum"]), _p(out["ssd"])))
        return out

    def performance_across_k(self, deltas, variances, n: int | None = None, d: int | None = None) -> dict:
        """``fk_performance_across_k``: float64 ``[n][d]`` chance deltas and variances (``batch_mcse ** 2``, squared by the caller as the
        reference squares it: ``performance.squared_mcse``) of the complete-support strategies, rows in ascending strategy id.  Returns
        float64 ``[n]`` ``delta_sum``, ``variance_sum``, ``minimum``, int32 ``worst_index``, bool ``pareto_member`` and ``leader_row``
        (``performance.host_across_k`` bit for bit).  ``n`` / ``d``: the shape handed to the entry when it is not the arrays'."""
        deltas = np.ascontiguousarray(deltas, dtype=np.float64)
        variances = np.ascontiguousarray(variances, dtype=np.float64)
        if deltas.ndim != 2 or deltas.shape != variances.shape:
            raise ValueError("deltas and variances are [n][d] arrays of one shape")
        n = deltas.shape[0] if n is None else int(n)
        d = deltas.shape[1] if d is None else int(d)
        rows = max(n, 0)
        out = {"delta_sum": np.zeros(rows), "variance_sum": np.zeros(rows), "minimum": np.zeros(rows), "worst_index": np.zeros(rows, np.int32)}
        member = np.zeros(rows, dtype=np.uint8)
        leader = C.c_int32(-1)
        self._check(self._lib.fk_performance_across_k(self._ctx, n, d, _p(deltas), _p(variances), _p(out["delta_sum"]), _p(out["variance_sum"]),
                                                      _p(out["minimum"]), _p(out["worst_index"]), _p(member), C.byref(leader)))
        out["pareto_member"], out["leader_row"] = member.astype(bool), int(leader.value)
        return out

    def root_window_estimates(self, wins, exposures, completed, safety, windows, S: int | None = None, batch_counts=None) -> dict:
        """``fk_root_window_estimates``: the two-root stability stage's sums over row windows of its cells.  ``wins[c]`` ..
        ``safety[c]``: the four int64 ``[B_c][S]`` matrices of cell ``c``, unprojected; ``windows``: int64 ``[n][4]`` rows ``(cell,
        row_begin, row_end, pairwise_begin)`` (``root_stability.window_pairwise_begin``).  Returns int64 ``[n][S]`` ``wins``,
        ``exposures``, ``completed``, ``safety``, ``losses``, ``positive_batches`` and float64 ``[n][S]`` ``sum_w2``, ``sum_we``,
        ``sum_e2`` (``root_stability.estimate_windows`` bit for bit).  ``S`` / ``batch_counts``: the shape handed to the entry when it
        is not the matrices' (refusal tests)."""
        kinds = [[np.ascontiguousarray(m, dtype=np.int64) for m in group] for group in (wins, exposures, completed, safety)]
        n_cells = len(kinds[0])
        if not n_cells or any(len(group) != n_cells for group in kinds):
            raise ValueError("one wins / exposures / completed / safety matrix per cell")
        width = int(kinds[0][0].shape[1]) if kinds[0][0].ndim == 2 else -1
        for cell in range(n_cells):
            if any(group[cell].ndim != 2 or group[cell].shape != kinds[0][cell].shape or group[cell].shape[1] != width for group in kinds):
                raise ValueError("every matrix is [batches][S] with one S, the four of a cell of one shape")
        windows = np.ascontiguousarray(windows, dtype=np.int64)
        if windows.ndim != 2 or windows.shape[1] != 4:
            raise ValueError("windows is [n][4]: cell, row_begin, row_end, pairwise_begin")
        S = width if S is None else int(S)
        b_arr = np.asarray([len(m) for m in kinds[0]] if batch_counts is None else batch_counts, dtype=np.int64)
        pointers = [(C.c_void_p * n_cells)(*[m.ctypes.data for m in group]) for group in kinds]
        n = len(windows)
        totals = np.zeros((n, len(ROOT_WINDOW_TOTALS), max(S, 0)), dtype=np.int64)
        sums = np.zeros((n, len(ROOT_WINDOW_SUMS), max(S, 0)), dtype=np.float64)
        self._check(self._lib.fk_root_window_estimates(self._ctx, n_cells, _p(b_arr), pointers[0], pointers[1], pointers[2], pointers[3], S, n,
                                                       _p(windows), _p(totals), _p(sums)))
        out = {name: totals[:, i, :] for i, name in enumerate(ROOT_WINDOW_TOTALS)}
        out.update({name: sums[:, i, :] for i, name in enumerate(ROOT_WINDOW_SUMS)})
        return out

    def debug_dice_state(self, state: np.ndarray, sizes):
        state = np.ascontiguousarray(state, dtype=np.uint64).reshape(-1, 6)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        n = len(state)
        faces = np.zeros((n, int(sizes.sum())), dtype=np.uint8)
        out = np.zeros((n, 6), dtype=np.uint64)
        self._check(self._lib.fk_debug_dice_state(self._ctx, n, _p(state), len(sizes), _p(sizes), _p(faces), _p(out)))
        return faces, out

    def debug_dice_keys(self, state: np.ndarray, sizes):
        """The game kernels' dice instantiation (``roll_counts<3>``) from explicit generator states: ``(keys[n][n_calls],
        state_out[n][6])``; key = six 3-bit face counts."""
        state = np.ascontiguousarray(state, dtype=np.uint64).reshape(-1, 6)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        n = len(state)
        keys = np.zeros((n, len(sizes)), dtype=np.uint32)
        out = np.zeros((n, 6), dtype=np.uint64)
        self._check(self._lib.fk_debug_dice_keys(self._ctx, n, _p(state), len(sizes), _p(sizes), _p(keys), _p(out)))
        return keys, out
