"""(CPU) The thresholds of tests/fog_adaptive_reference.py's settings, by a sweep on the restatements: for each setting the value whose
least-populated stop level (of the eight, 4 … 32) is fullest, and the pixels per level there.
  python3 tools/fog_adaptive_sweep.py [setting …]
  python3 tools/fog_adaptive_sweep.py --fuzz      the mid thresholds of tests/test_fog_adaptive_fuzz.py: per family the value under which
                                                  the most trials have two levels of at least 5 pixels (ties: the fullest second level)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ray-tracing-practice_amd"), os.path.join(ROOT, "tests")]

import fog_adaptive_reference as far  # noqa: E402

GRID = [round(x, 3) for x in np.concatenate([np.arange(0.02, 0.1, 0.01), np.arange(0.1, 0.5, 0.025), np.arange(0.5, 2.01, 0.1)])]


def fuzz():
    import lit_fuzz as lf
    import test_fog_adaptive_fuzz as fz
    for family in fz.FAMILIES:
        def score(t):
            counts = [fz.level_counts(trial, family, t) for trial in lf.TRIALS]
            return sum(sum(n >= 5 for n in c) >= 2 for c in counts), sum(sorted(c)[-2] for c in counts)
        best = max(GRID, key=score)
        counts = {trial: fz.level_counts(trial, family, best) for trial in lf.TRIALS}
        print(f"{family!r}: threshold {best}  trials with two levels of >= 5 pixels: {score(best)[0]}  pixels per level (3, 5, 7, 9) by trial: {counts}", flush=True)


def main():
    if sys.argv[1:] == ["--fuzz"]:
        return fuzz()
    for setting in sys.argv[1:] or list(far.SETTINGS):
        best = max(GRID, key=lambda t: (min(far.level_counts(setting, t)), -t))
        counts = far.level_counts(setting, best)
        print(f"{setting!r}: threshold {best}  levels {dict(zip(far.LEVELS, counts))}  smallest {min(counts)}", flush=True)


if __name__ == "__main__":
    main()
