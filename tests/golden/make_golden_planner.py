"""Generate tests/golden/rs_planner_quirks.npz by RUNNING the reference's RsPlanner (build container only).

    python tests/golden/make_golden_planner.py --reference <checkout of jiamiya/HOPE>

RsPlanner.set_rs_path (src/model/agent/parking_agent.py:12-41) is fed paths whose segment lengths sit on the edges of its rule,
with step_ratio = 0.05 * 10 * 2.5 as the training scripts pass it.  The fixture holds numbers only, in the layout of
agent_glue.npz's planner part --

  words [M][5] int8        segment types (0 S, 1 L, 2 R; -1 unused)
  lengths [M][5] float64   signed segment lengths in metres
  actions [T][2] float64   the concatenated action lists, action_off [M + 1] their offsets

The edge lengths (each with both signs, and each once more rounded to float32): one step exactly (dropped), two and three steps
(the remainder is exactly +-1), one step +- one ulp, the 1e-3 keep threshold and its two float64 neighbours, one step plus the
threshold and its neighbours, and +-0.  They appear in one-, three- and five-segment words."""
import argparse
import importlib.util
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEP_RATIO = 0.05 * 10 * 2.5
CODE = {'S': 0, 'L': 1, 'R': 2}


def quirk_lengths():
    r = STEP_RATIO
    nb = lambda v: [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]  # noqa: E731
    q = [r, 2 * r, 3 * r, r * (1 + 2.0 ** -52), r * (1 - 2.0 ** -52)] + nb(r * 1e-3) + nb(r * (1 + 1e-3)) + [0.0]
    q = q + [-v for v in q]
    q = q + [float(np.float32(v)) for v in q]
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(HERE, 'rs_planner_quirks.npz'))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location('ref_parking_agent', os.path.join(a.reference, 'src', 'model', 'agent', 'parking_agent.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    q = quirk_lengths()
    paths = []
    for i, v in enumerate(q):
        w = q[(i + 7) % len(q)]
        paths.append(('LSR'[i % 3], [v]))
        paths.append((['LSR', 'RSL', 'LRL', 'RLR'][i % 4], [v, 2.0, -v]))
        paths.append((['LSLSR', 'RSRSL', 'LRSLR', 'RLSRL'][i % 4], [v, -0.7, w, 3.1, -v]))
        paths.append((['LRSRL', 'SLSRS'][i % 2], [0.3, v, v, -w, 1.9]))
    words = np.full((len(paths), 5), -1, np.int8)
    lengths = np.zeros((len(paths), 5))
    acts, off = [], [0]
    for k, (ct, ln) in enumerate(paths):
        words[k, :len(ct)] = [CODE[c] for c in ct]
        lengths[k, :len(ln)] = ln
        pl = mod.RsPlanner(STEP_RATIO)
        pl.set_rs_path(types.SimpleNamespace(ctypes=list(ct), lengths=[float(x) for x in ln]))
        acts.extend([float(s), float(x)] for s, x in pl.actions)
        off.append(len(acts))
    np.savez_compressed(a.out, words=words, lengths=lengths, actions=np.array(acts, np.float64).reshape(-1, 2), action_off=np.array(off, np.int64))
    print(f'{len(paths)} paths, {len(acts)} actions -> {a.out}')


if __name__ == '__main__':
    main()
