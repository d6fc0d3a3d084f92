"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, exports every
symbol include/farkle_hip.h declares, and fails loudly (no CPU fallback) when no GPU is present.  The Python side of the ABI
(farkle_ii_amd/backend.py) is checked against the header here as well: the signatures it parses, the arity of its call sites, its copies of
the header's constants and its mirrors of the header's structs."""
from __future__ import annotations

import ast
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEADER_TEXT = (ROOT / "include" / "farkle_hip.h").read_text()
HEADER_CODE = re.sub(r"/\*.*?\*/", " ", HEADER_TEXT, flags=re.S)  # (comments name fields and constants too)


def test_library_builds_and_exports_every_declared_symbol():
    from farkle_ii_amd import backend

    backend.build_library()
    lib = backend.load_library()
    declared = set(re.findall(r"^(?:int|void|size_t|const char \*)\s*\*?(fk_\w+)\(", HEADER_TEXT, flags=re.M))
    assert {"fk_init", "fk_tournament_run", "fk_play_games", "fk_h2h_run", "fk_last_error", "fk_destroy"} <= declared
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/farkle_hip.h but not exported"
    assert declared == set(backend.signatures())  # the declared set is the parsed set: load_library typed every one of them
    for name, (restype, argtypes) in backend.signatures().items():
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name


def test_struct_layouts_match_header():
    from farkle_ii_amd import backend
    from farkle_ii_amd.strategies import STRATEGY_DTYPE

    assert STRATEGY_DTYPE.itemsize == 20 and backend.SEAT_DTYPE.itemsize == 28
    assert backend.COORD_DTYPE.itemsize == 72 and backend.OVERRIDE_DTYPE.itemsize == 32
    for k in (1, 2, 4, 12):
        assert backend.row_dtype(k).itemsize == 4 + 28 * k


def test_no_cpu_fallback_without_gpu():
    import torch

    from farkle_ii_amd.backend import Engine, FarkleHipError

    if torch.cuda.is_available():
        pytest.skip("GPU present: the loud-failure path is for GPU-less hosts")
    with pytest.raises(FarkleHipError, match="no usable HIP device|HIP runtime"):
        Engine(0)


def test_product_never_touches_the_oracle():
    """The oracle is test infrastructure: nothing under farkle_ii_amd/ may import, load or link it."""
    for path in (ROOT / "farkle_ii_amd").rglob("*"):
        if path.suffix in {".py", ".hip", ".h", ".cpp"}:
            text = path.read_text()
            assert "pyoracle" not in text and "liboracle" not in text and "farkle_oracle" not in text, path


def test_comm_init_deadline_handshake_has_exactly_one_owner():
    """fk_comm_init runs ncclCommInitRank on a helper thread under a deadline.  Whatever the timing — the initialisation returning long
    before, long after or AT the deadline — the communicator ends up with exactly one owner: the caller received it, or the helper tore it
    down as an orphan; never both (the round-5 two-flag handshake could install a communicator that was being aborted), never neither."""
    import ctypes as C

    import numpy as np

    from farkle_ii_amd.backend import load_library

    lib = load_library()
    out = np.zeros(2, dtype=np.int64)
    received = {}
    for init_ms in (0, 5, 18, 19, 20, 21, 22, 45):
        for _ in range(10):
            assert lib.fk_debug_deadline_handshake(C.c_int32(init_ms), C.c_int32(20), out.ctypes.data_as(C.c_void_p)) == 0
            assert int(out[0]) + int(out[1]) == 1, (init_ms, out.tolist())
            received[init_ms] = received.get(init_ms, 0) + int(out[0])
    assert received[0] == received[5] == 10 and received[45] == 0  # (the timings around 20 ms may go either way: that is the point)


def test_signature_parse_fails_loudly():
    """A by-value type without a ctypes mapping, or a prototype the pattern cannot read, stops the load: no function is skipped."""
    from farkle_ii_amd import backend

    sig = backend.parse_signatures(HEADER_TEXT)
    assert sig == backend.signatures() and len(sig) >= 63
    assert sig["fk_set_option"] == (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64])
    assert sig["fk_h2h_run"][1] == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    assert sig["fk_row_columns_bytes"] == (C.c_size_t, [C.c_int32, C.c_int32]) and sig["fk_destroy"] == (None, [C.c_void_p])
    assert sig["fk_last_error"] == (C.c_char_p, [C.c_void_p]) and sig["fk_write_row_shards"][1][4:] == [C.c_void_p, C.c_size_t]
    one = "int fk_rows_wait(fk_ctx *ctx, int32_t slot);"
    assert one in HEADER_TEXT
    with pytest.raises(ValueError, match="fk_rows_wait.*float gain"):
        backend.parse_signatures(HEADER_TEXT.replace(one, "int fk_rows_wait(fk_ctx *ctx, int32_t slot, float gain);"))
    with pytest.raises(ValueError, match="begin like a prototype"):  # a return type the table does not know: seen, not matched
        backend.parse_signatures(HEADER_TEXT.replace(one, "int *fk_rows_wait(fk_ctx *ctx, int32_t slot);"))
    with pytest.raises(ValueError, match="begin like a prototype"):  # a callback parameter
        backend.parse_signatures(HEADER_TEXT.replace(one, "int fk_rows_wait(fk_ctx *ctx, void (*done)(int32_t));"))
    with pytest.raises(ValueError, match="begin like a prototype"):  # declared twice
        backend.parse_signatures(HEADER_TEXT + one)


def _fk_calls(tree):
    """(entry name, call node) of every ``<something>.fk_*(...)`` call below ``tree``."""
    return [(node.func.attr, node) for node in ast.walk(tree)
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("fk_")]


def _backend_tree():
    from farkle_ii_amd import backend

    return ast.parse(Path(backend.__file__).read_text())


def test_every_lead_entry_starts_with_the_same_thirteen_parameters():
    """``Engine._lead`` is unpacked into every tournament entry: they must agree on those parameters, and ``_lead`` on their number."""
    import numpy as np

    from farkle_ii_amd import backend
    from farkle_ii_amd.strategies import STRATEGY_DTYPE

    sig = backend.signatures()
    through_lead = {"fk_tournament_run"}  # (tests/test_wide_tables_gpu.py calls it with Engine._lead)
    for fn in ast.walk(_backend_tree()):
        if isinstance(fn, ast.FunctionDef) and any(isinstance(n, ast.Attribute) and n.attr == "_lead" for n in ast.walk(fn)):
            through_lead |= {name for name, call in _fk_calls(fn) if any(isinstance(a, ast.Starred) for a in call.args)}
    assert through_lead == {"fk_tournament_run", "fk_tournament_run_stats", "fk_tournament_run_all_player", "fk_tournament_run_game_stats",
                            "fk_tournament_run_rare_events", "fk_tournament_run_seat_counts", "fk_tournament_run_columns",
                            "fk_tournament_run_columns_seeds", "fk_tournament_run_lags", "fk_tournament_run_matchups"}
    assert "fk_tournament_run_census" not in through_lead  # (it takes no tally: Engine.tournament_census spells its arguments out)
    common = sig["fk_tournament_run"][1][:13]
    assert common == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32,
                      C.c_void_p, C.c_int32, C.c_void_p]
    for name in through_lead:
        assert sig[name][1][:13] == common, name
    eng = object.__new__(backend.Engine)  # (no context: _lead only packs)
    eng._ctx = C.c_void_p()
    lead = eng._lead(np.zeros(4, STRATEGY_DTYPE), 4, 2, 42, 0, np.int64(3), 3, 10_000, 200, np.zeros(1, backend.OVERRIDE_DTYPE),
                     np.zeros((1, 4, backend.TALLY_COLS), np.int64))
    assert len(lead) == 13
    for value, kind in zip(lead, common):
        kind.from_param(value)  # every value is one its parameter takes


def test_every_unstarred_call_site_has_the_header_arity():
    """ctypes refuses a call with too few arguments but lets extra ones through (cdecl), so the count is checked here, statically."""
    from farkle_ii_amd import backend

    sig = backend.signatures()
    checked = set()
    for name, call in _fk_calls(_backend_tree()):
        assert name in sig, f"backend.py calls {name}, which include/farkle_hip.h does not declare"
        assert not call.keywords, name
        if not any(isinstance(a, ast.Starred) for a in call.args):
            assert len(call.args) == len(sig[name][1]), f"line {call.lineno}: {name} takes {len(sig[name][1])} arguments, the call passes {len(call.args)}"
            checked.add(name)
    assert len(checked) >= 45 and {"fk_init", "fk_h2h_run", "fk_tournament_run_census", "fk_write_row_shards", "fk_rr_root_diagnostics"} <= checked


def _header_constants() -> dict:
    defines = {name: int(value) for name, value in re.findall(r"^#define (FK_\w+) (-?\d+)\s*$", HEADER_CODE, flags=re.M)}
    errors = re.search(r"enum \{\s*(FK_OK = 0,.*?)\}", HEADER_CODE, flags=re.S).group(1)
    return {**defines, **{name: int(value) for name, value in re.findall(r"(FK_\w+) = (-?\d+)", errors)}}


def test_python_copies_of_the_header_constants():
    from farkle_ii_amd import backend, roll_census, round_robin, rr_root_diagnostics, trace

    fk = _header_constants()
    pairs = [(backend.TALLY_COLS, "FK_TALLY_COLS"), (backend.SEAT_STAT_COLS, "FK_SEAT_STAT_COLS"), (backend.SEAT_RATIO_COLS, "FK_SEAT_RATIO_COLS"),
             (backend.LAG_COLS, "FK_LAG_COLS"), (backend.RR_MAX_ROOTS, "FK_RR_MAX_ROOTS"), (backend.RR_AGREE_COLS, "FK_RR_AGREE_COLS"),
             (backend.RR_CLASSES, "FK_RR_CLASSES"), (backend.RR_STRATEGY_COLS, "FK_RR_STRATEGY_COLS"), (backend.DOM_MAX_N, "FK_DOM_MAX_N"),
             (backend.AGREE_COUNTS, "FK_AGREE_COUNTS"), (backend.AGREE_NO_RANK, "FK_AGREE_NO_RANK"),
             (backend.CONCORDANCE_COUNTS, "FK_CONCORDANCE_COUNTS"), (backend.CONCORDANCE_MAX_M, "FK_CONCORDANCE_MAX_M"),
             (backend.CONCORDANCE_TILE, "FK_CONCORDANCE_TILE"), (backend.FK_ERR_ROLL_LIMIT, "FK_ERR_ROLL_LIMIT"), (backend.FK_ERR_ARG, "FK_ERR_ARG"),
             (backend.FK_ERR_COUNTER_OVERFLOW, "FK_ERR_COUNTER_OVERFLOW"), (backend.FK_ERR_HIP, "FK_ERR_HIP"),
             (backend.FK_ERR_NO_DEVICE, "FK_ERR_NO_DEVICE"), (backend.FK_ERR_COMM, "FK_ERR_COMM"), (backend.FK_ERR_IO, "FK_ERR_IO"),
             (len(round_robin.STATE_COLS), "FK_RR_STATE_COLS"), (len(round_robin.SUMMARY_COLS), "FK_RR_SUMMARY_COLS"),
             (rr_root_diagnostics.DECISION_NONE, "FK_RR_DIAGNOSTIC_NONE"), (roll_census.EV_ROLL_AGAIN, "FK_EV_ROLL_AGAIN"),
             (len(backend.SEAT_STAT_NAMES), "FK_SEAT_STAT_COLS"), (trace.EV_DECIDE, "FK_EV_DECIDE"), (trace.EV_ROLL_AGAIN, "FK_EV_ROLL_AGAIN"),
             (trace.EV_FINAL_ROUND, "FK_EV_FINAL_ROUND"), (trace.EV_AUTO_HOT, "FK_EV_AUTO_HOT")]
    assert fk["FK_OK"] == 0 and fk["FK_ERR_IO"] == -7 and fk["FK_DOM_MAX_N"] == 8192  # (the parse reads values, not just names)
    wrong = [f"{name}: the header says {fk[name]}, Python {value}" for value, name in pairs if fk[name] != value]
    assert not wrong, "\n".join(wrong)
    assert {name for name in fk if name.startswith("FK_ERR_")} == {name for _, name in pairs if name.startswith("FK_ERR_")}  # every code has a name


def _header_structs() -> dict:
    """``{struct: [field names, in order]}`` of every ``typedef struct { ... } fk_*;`` of the header."""
    structs = {}
    for body, name in re.findall(r"typedef struct \{(.*?)\}\s*(fk_\w+);", HEADER_CODE, flags=re.S):
        pieces = [piece for decl in body.split(";") for piece in decl.split(",") if piece.strip()]
        structs[name] = [re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", piece).group(1) for piece in pieces]
    return structs


def _mirror_fields(mirror) -> tuple:
    """(size, [(field, offset, size)]) of a NumPy dtype or a ctypes Structure."""
    if isinstance(mirror, np.dtype):
        return mirror.itemsize, [(n, mirror.fields[n][1], mirror.fields[n][0].itemsize) for n in mirror.names]
    return C.sizeof(mirror), [(n, getattr(mirror, n).offset, getattr(mirror, n).size) for n, *_ in mirror._fields_]


def test_every_header_struct_has_a_mirror_of_its_layout(tmp_path):
    """A host program generated from the header's own struct bodies prints sizeof and every field's offsetof / size; each Python mirror
    must say the same, field by field and in order.  A field added, removed or moved in the header, or a struct without a mirror, fails."""
    from farkle_ii_amd import backend
    from farkle_ii_amd.strategies import STRATEGY_DTYPE

    structs = _header_structs()
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "farkle_hip.h"', "int main() {"]
    for name, fields in structs.items():
        lines.append(f'    std::printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    std::printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));' for f in fields]
    source = tmp_path / "abi_layout_check.hip"
    source.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    exe = tmp_path / "abi_layout_check"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-I", str(ROOT / "include"), "-o", str(exe), str(source)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    header, words = {}, iter(out)
    for word in words:
        struct, _, field = word.partition(".")
        if field:
            header[struct][1].append((field, int(next(words)), int(next(words))))
        else:
            header[struct] = (int(next(words)), [])
    assert {name: [f for f, _, _ in fields] for name, (_, fields) in header.items()} == structs  # the program printed what the header declares

    mirrors = {"fk_strategy": STRATEGY_DTYPE, "fk_seat": backend.SEAT_DTYPE, "fk_override": backend.OVERRIDE_DTYPE, "fk_coord": backend.COORD_DTYPE,
               "fk_device_info": backend._DeviceInfo, "fk_timing": backend._Timing, "fk_shard_job": backend._ShardJob,
               "fk_roll_event": backend.EVENT_DTYPE, "fk_census": backend._Census, "fk_h2h_block": backend.H2H_BLOCK_DTYPE,
               "fk_rr_inference_params": backend._RrInferenceParams, "fk_rr_pair_row": backend.RR_PAIR_ROW_DTYPE,
               "fk_rr_root_row": backend.RR_ROOT_ROW_DTYPE, "fk_rr_agreement_row": backend.RR_AGREEMENT_ROW_DTYPE,
               "fk_dom_node": backend.DOM_NODE_DTYPE, "fk_dom_extreme": backend.DOM_EXTREME_DTYPE}
    partial = {"fk_row_hdr", "fk_comm_id"}  # the head of row_dtype(k) and COMM_ID_BYTES, below
    assert set(header) == set(mirrors) | partial, "a struct of include/farkle_hip.h without a Python mirror (or a mirror of no struct)"
    assert len(mirrors) == 16 and len(header) == 18
    for name, mirror in mirrors.items():
        assert _mirror_fields(mirror) == header[name], name
    for k in (1, 2, 12):
        size, fields = _mirror_fields(backend.row_dtype(k))
        assert fields[:3] == header["fk_row_hdr"][1] and len(header["fk_row_hdr"][1]) == 3
        assert fields[3] == ("seats", header["fk_row_hdr"][0], k * header["fk_seat"][0]) and size == header["fk_row_hdr"][0] + k * header["fk_seat"][0]
    assert header["fk_comm_id"] == (backend.COMM_ID_BYTES, [("bytes", 0, backend.COMM_ID_BYTES)])
