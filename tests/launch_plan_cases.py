"""The inputs of the launch-plan fixture (tests/golden/launch_plan.json) and the program that plans them (test helper, not a conftest).

The planner of the game kernel's launch (csrc/fk_plan.h) is a pure host function of the seat count, the table size, the target, the call's
mode, a handful of options and the CU count.  ``inputs()`` lists the calls the fixture pins, in the fixture's order; ``run_planner`` builds
tests/native/launch_plan_host_check.hip and returns one plan per input.  tools/gen_launch_plan_golden.py wrote the fixture with both;
tests/test_launch_plan_host.py compares the present planner with it.
"""
from __future__ import annotations

import os
import subprocess
from pathlib import Path
from typing import NamedTuple

import kernel_instances as ki

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = ROOT / "tests" / "native" / "launch_plan_host_check.hip"
FIXTURE = ROOT / "tests" / "golden" / "launch_plan.json"

MODES = ("tournament", "list", "h2h_blocks")
# the options of fk_set_option the planner reads, at the defaults of a fresh context (farkle_hip.hip: fk_ctx), which are the Engine's
DEFAULTS = {"max_waves": 6, "blocks_per_cu": 0, "block": 0, "lean": -1, "state_store": -1, "hot_cold": -1, "use_lds_tally": -1}
PLAN_FIELDS = ("block", "grid", "lds", "lds_tally", "lean", "gs", "blk", "hc", "shape")


class Input(NamedTuple):
    mode: str
    cus: int
    k: int
    S: int
    single_batch: int
    target: int
    options: tuple  # (name, value) pairs that differ from DEFAULTS

    def line(self) -> str:
        o = {**DEFAULTS, **dict(self.options)}
        return " ".join(str(v) for v in (MODES.index(self.mode), self.cus, self.k, self.S, self.single_batch, self.target,
                                         *(o[name] for name in DEFAULTS)))


CUS = (256, 7)
SEATS = (*range(1, 14), 16, 32, 33, 64, 65, 128)
TABLE_FLOORS = (96, 4097, 5160, 16385)  # the tests' size; past the LDS-tally limit; production; past the lean records' 14-bit index
TARGETS = (1500, 10_000, 135_000, 135_050, 3_200_050)  # ..., the hot / cold limit, just past it, just past the lean-record limit
OPTION_SETTINGS = ((), *((("max_waves", v),) for v in (1, 3, 4, 8)), *((("blocks_per_cu", v),) for v in (1, 2)),
                   *((("lean", v),) for v in (0, 1)), *((("block", v),) for v in (64, 128, 256, 512, 768, 1024)),
                   (("state_store", 1),), (("hot_cold", 0),), (("use_lds_tally", 0),))


def table_size(k: int, floor: int) -> int:
    return -(-floor // k) * k


def inputs() -> list[Input]:
    out = [Input("tournament", cus, k, table_size(k, floor), single, target, options)
           for cus in CUS for k in SEATS for floor in TABLE_FLOORS for target in TARGETS for single in (0, 1) for options in OPTION_SETTINGS]
    # every option tuple of the routes (tests/kernel_instances.py), at the route's own seats and table
    for route in ki.SHAPES.values():
        options = tuple((n, v) for n, v in route.options if n in DEFAULTS)
        assert len(options) == len(route.options), route
        for cus in CUS:
            if route.entry == "h2h_blocks":
                out.append(Input("h2h_blocks", cus, route.k, route.S, 0, 10_000, options))
            else:
                out += [Input("tournament", cus, route.k, route.S, single, 10_000, options) for single in (0, 1)]
                out.append(Input("list", cus, route.k, route.S, 0, 10_000, options))
    out += [Input("h2h_blocks", cus, 2, 96, 0, target, (("blocks_per_cu", v),) if v else ())
            for cus in CUS for target in (10_000, 3_200_050) for v in (0, 1, 2)]
    return out


def build_planner(directory: Path, source: Path = SOURCE) -> Path:
    """The stand-alone host program: host side only (the planner runs no device code), so one quick hipcc call."""
    exe = Path(directory) / "launch_plan_host_check"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-o", str(exe), str(source)], check=True,
                   capture_output=True, text=True)
    return exe


def run_planner(exe: Path, cases: list[Input]) -> list[dict | None]:
    """One plan per input, ``None`` where no instance fits: the fields of ``PLAN_FIELDS``, the shape as tests/kernel_instances.py spells it."""
    out = subprocess.run([str(exe)], input="".join(c.line() + "\n" for c in cases), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases), (len(lines), len(cases))
    plans = []
    for text in lines:
        if text == "none":
            plans.append(None)
            continue
        numbers, shape = text.split(" ", len(PLAN_FIELDS) - 1)[:-1], text.split(" ", len(PLAN_FIELDS) - 1)[-1]
        plans.append({**{name: int(v) for name, v in zip(PLAN_FIELDS, numbers)}, "shape": shape})
    return plans


def check_conditions(cases: list[Input], plans: list[dict | None]) -> None:
    """What the fixture must cover: all 21 shapes, a call without an instance, and not mostly such calls."""
    named = {p["shape"] for p in plans if p is not None}
    assert named == set(ki.SHAPES), (sorted(set(ki.SHAPES) - named), sorted(named - set(ki.SHAPES)))
    none = sum(p is None for p in plans)
    assert 1 <= none and 10 * none <= len(plans), (none, len(plans))
