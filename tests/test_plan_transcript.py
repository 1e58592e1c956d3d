"""The launch policy's answers, recorded: grail_plan_blocks and grail_plan_ragged_blocks over a fixed grid of batch sizes,
arithmetics, formant counts, device sizes, spans and warm-up lengths, one line per plan with every field of every block
(model_ms as float.hex()).  tests/golden/plan_transcript.txt is what the library answered before the planner's input
became types of its own (BatchFacts, PlanEnv); a change of the host code that is not meant to move a plan must repeat it
byte for byte.  No GPU needed.  Run as a script, the module writes the transcript (to the path given, else to stdout)."""
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "grail-rs_amd"), os.path.join(_root, "tests")]

import grail_hip as G
from test_plan import _speech_like_rows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_transcript.txt")

ROWS = (1, 64, 300, 1024, 1025, 4096, 8704, 20000, 65536, 70000, 131072)
RAGGED_ROWS = (300, 4096, 20000, 70000)
ARITHMETIC = (0, 1, 2)
FORMANTS = (4, 8)
CUS = (256, 32, 20)
SPANS = (8000, 96006)
WARMUPS = (0, 3904)


def _cells():
    """(compute units, arithmetic, formants, span, warm-up): every value of every axis; the whole product on the whole
    device, the two smaller devices at the long span and the usual warm-up.  (Exact arithmetic never reads the warm-up.)"""
    for cus in CUS:
        for arith in ARITHMETIC:
            for formants in FORMANTS:
                for span in (SPANS if cus == 256 else SPANS[1:]):
                    for warmup in (WARMUPS if cus == 256 and arith else WARMUPS[1:]):
                        yield cus, arith, formants, span, warmup


def _blocks(plan):
    return ";".join(f"{b.rows},{b.lanes_per_utterance},{b.pipelined},{b.chunks},{b.scan},{b.fast},{b.formants},"
                    f"{float(b.model_ms).hex()}" for b in plan)


def transcript():
    lines = []
    for cus, arith, formants, span, warmup in _cells():
        for rows in ROWS:
            plan = G.plan_blocks(rows, span, arith, formants, warmup=warmup, compute_units=cus)
            lines.append(f"aligned cus={cus} a={arith} f={formants} span={span} w={warmup} rows={rows}: {_blocks(plan)}")
    speech = {rows: _speech_like_rows(rows) for rows in RAGGED_ROWS}
    for cus in CUS:
        for arith in ARITHMETIC:
            for formants in FORMANTS:
                for warmup in (WARMUPS if arith else WARMUPS[1:]):
                    for rows in RAGGED_ROWS:
                        samples, segs, kinks = speech[rows]
                        plan = G.plan_ragged_blocks(samples, segs, kinks, arithmetic=arith, live_formants=formants,
                                                    warmup=warmup, compute_units=cus)
                        lines.append(f"speech cus={cus} a={arith} f={formants} w={warmup} rows={rows}: {_blocks(plan)}")
    return "\n".join(lines) + "\n"


def test_every_plan_of_the_grid_repeats_the_recorded_transcript():
    got = transcript()
    recorded = open(GOLDEN).read()
    assert len(recorded) < 64 * 1024 and recorded.count("\n") == len(got.splitlines())
    for a, b in zip(got.splitlines(), recorded.splitlines()):
        assert a == b
    assert got == recorded


if __name__ == "__main__":
    text = transcript()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
