"""TEST INFRASTRUCTURE ONLY — write tests/golden/watch_vectors.json by running the upstream Python reference in the build
container (oracle/ref_import.py; nothing here travels to the GPU machine except the JSON).

(a) ``watch_game(seed)`` of the reference (src/farkle/simulation/watch_game.py:157-221), its log messages captured with a
    logging handler: in full for seeds 47 and 6 (the shortest of seeds 0-299), 42, 12 and 25 (the final-turn player overtakes: the
    last ``score(...)`` line has no ``decide()`` line behind it; seed 25 also has a ``reroll=0`` roll followed by ``dice_left=6``);
    as message count + SHA-256 of ``"\\n".join(messages)`` for seed 7 and — up to and including the ``final result`` line, the
    reference cannot format the record behind it — for seed 253, a 200-round safety-limit game.
(b) two three-player games of scripted strategies, composed from the reference's own ``TracePlayer``, ``patch_scoring``,
    ``_trace_decide`` and ``FarkleGame`` with the seat streams of namespace 103 and ``target_score=2000``: one table with
    ``auto_hot_dice``, one with ``run_up_score`` and both smart discards (``random_threshold_strategy`` sets neither flag).  Each
    is the first (shuffle, game), in the order shuffle = n // 8, game = n % 8, at which the flag's event occurs: an auto-hot-dice
    roll; a discard and a ``decide()`` in the final round above the score to beat.

    python tools/gen_watch_golden.py
"""
from __future__ import annotations

import hashlib
import json
import logging
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "oracle"))
import gen_golden as gg  # noqa: E402  (imports the reference through oracle/ref_import.py)

from farkle.game.engine import FarkleGame  # noqa: E402
from farkle.simulation import watch_game as wg  # noqa: E402
from farkle.simulation.strategies import random_threshold_strategy  # noqa: E402

OUT = HERE.parent / "tests" / "golden" / "watch_vectors.json"
FULL_SEEDS, DIGEST_SEEDS = (47, 6, 42, 12, 25), (7, 253)
TARGET_B, K_B = 2000, 3


class Capture(logging.Handler):
    """The formatted messages of the watch logger; a record that cannot be formatted ends the capture (seed 253's last one)."""

    def __init__(self):
        super().__init__(level=logging.DEBUG)
        self.messages: list[str] = []
        self.failed = False

    def emit(self, record):
        assert getattr(record, "stage", None) == "watch"
        if self.failed:
            return
        try:
            self.messages.append(record.getMessage())
        except TypeError:
            self.failed = True


def captured(fn):
    handler = Capture()
    wg.LOGGER.addHandler(handler)
    level, propagate = wg.LOGGER.level, wg.LOGGER.propagate
    wg.LOGGER.setLevel(logging.INFO)
    wg.LOGGER.propagate = False
    try:
        result = fn()
    finally:
        wg.LOGGER.removeHandler(handler)
        wg.LOGGER.setLevel(level)
        wg.LOGGER.propagate = propagate
    return handler, result


def digest(messages) -> str:
    return hashlib.sha256("\n".join(messages).encode()).hexdigest()


def watch_case(seed: int) -> dict:
    handler, _ = captured(lambda: wg.watch_game(seed))
    strategies = [random_threshold_strategy(gg.ur.coordinate_rng(gg.RandomPurpose.STRATEGY, root_seed=seed, k=2, seat_index=i)) for i in range(2)]
    case = {"seed": seed, "strategies": [gg.strat_tuple(s) for s in strategies], "count": len(handler.messages),
            "sha256": digest(handler.messages), "truncated": handler.failed}
    if seed in FULL_SEEDS:
        case["messages"] = handler.messages
    return case


def scripted_game(strategies, root_seed: int, shuffle: int, game: int):
    """One game of `strategies` (fresh copies) through the reference's tracing wrappers; also what its seats did."""
    import copy

    strategies = [copy.copy(s) for s in strategies]
    run_ups = []
    for i, s in enumerate(strategies):
        plain = s.decide

        def spying(plain=plain, **kw):  # sees what _trace_decide's wrapper passes on
            if kw.get("final_round") and kw.get("running_total", 0) > kw.get("score_to_beat", 0):
                run_ups.append(1)
            return plain(**kw)

        s.decide = spying
        wg._trace_decide(s, f"P{i + 1}")

    def play():
        with wg.patch_scoring():
            players = [wg.TracePlayer(f"P{i + 1}", s, rng=gg.ur.coordinate_rng(gg.RandomPurpose.TOURNAMENT_PLAYER, root_seed=root_seed, k=K_B,
                                                                              shuffle_index=shuffle, game_index=game, seat_index=i))
                       for i, s in enumerate(strategies)]
            return players, FarkleGame(players, target_score=TARGET_B).play()

    handler, (players, metrics) = captured(play)
    assert not handler.failed
    seen = {"hot_dice": sum(p.n_hot_dice for p in players), "discards": sum(p.smart_five_uses + p.smart_one_uses for p in players),
            "run_ups": len(run_ups)}
    outcome = {"winner": metrics.winner, "winning_score": metrics.winning_score, "n_rounds": metrics.n_rounds,
               "scores": [p.score for p in players], "rolls": [p.n_rolls for p in players]}
    return handler.messages, seen, outcome


def scripted_case(name: str, strategies, root_seed: int, wanted) -> dict:
    for n in range(4096):
        shuffle, game = n // 8, n % 8
        messages, seen, outcome = scripted_game(strategies, root_seed, shuffle, game)
        if all(seen[w] > 0 for w in wanted):
            return {"name": name, "root_seed": root_seed, "k": K_B, "purpose": int(gg.RandomPurpose.TOURNAMENT_PLAYER), "shuffle": shuffle,
                    "game": game, "target": TARGET_B, "max_rounds": 200, "strategies": [gg.strat_tuple(s) for s in strategies],
                    "seen": seen, "outcome": outcome, "count": len(messages), "sha256": digest(messages), "messages": messages}
    raise SystemExit(f"{name}: no game with {wanted} among the first 4096")


def main() -> None:
    T = gg.ThresholdStrategy
    F = gg.FavorDiceOrScore
    hot = [T(300, 2, auto_hot_dice=True), T(500, 1, smart_five=True, auto_hot_dice=True), T(400, 3, require_both=True, auto_hot_dice=True)]
    run_up = [T(350, 2, smart_five=True, smart_one=True, run_up_score=True, favor_dice_or_score=F.DICE),
              T(600, 1, smart_five=True, smart_one=True, run_up_score=True, require_both=True),
              T(450, 3, smart_five=True, smart_one=True, run_up_score=True, consider_dice=False)]
    out = {"digest": 'sha256("\\n".join(messages))',
           "watch": [watch_case(seed) for seed in FULL_SEEDS + DIGEST_SEEDS],
           "scripted": [scripted_case("auto_hot_dice", hot, 5, ("hot_dice",)), scripted_case("run_up_score", run_up, 5, ("discards", "run_ups"))]}
    OUT.write_text(json.dumps(out, cls=gg._Enc, separators=(",", ":")))  # (_Enc: NumPy scalars)
    for case in out["watch"]:
        print("watch", case["seed"], case["count"], "truncated" if case["truncated"] else "")
    for case in out["scripted"]:
        print(case["name"], (case["shuffle"], case["game"]), case["count"], case["seen"], case["outcome"])
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
