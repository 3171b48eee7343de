"""Generate tests/golden/curriculum.npz by RUNNING the reference's two chooser classes (build container only).

    python tests/golden/make_golden_curriculum.py --reference <checkout of jiamiya/HOPE>

SceneChoose and DlpCaseChoose (src/train/train_HOPE_sac.py:23-97) need numpy only, but their module imports matplotlib, torch and
tensorboard and starts a training run, so the two class definitions are cut out of the module's syntax tree and executed on their
own, unmodified.  Nothing of their text is written anywhere: the fixture holds numbers only --

  type_hist_n / type_hist_s [H][4]   records / successes among the last 250 records of each scene type in history h
  type_p [H][4]                      the p vector _choose_case_worst_perform handed to np.random.choice for that history
  case_hist_n / case_hist_s [H][248] records / successes among the last 10 records of each case (n = total records when <= 1)
  case_p [H][248]                    the p vector DlpCaseChoose.choose_case handed to np.random.choice
  freq_hist_n / freq_hist_s [F][4], freq [F][4]   frozen type histories and SceneChoose.choose_case's type frequencies over
                                     `freq_choices` choices each (no record is fed back while counting)
  freq_margin                        the largest |frequency - q| seen, q from hope_amd.curriculum.type_q: the test allows twice that
"""
import argparse
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def load_choosers(ref):
    path = os.path.join(ref, 'src', 'train', 'train_HOPE_sac.py')
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ('SceneChoose', 'DlpCaseChoose')]
    assert len(keep) == 2
    ns = {'np': np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, 'exec'), ns)
    return ns['SceneChoose'], ns['DlpCaseChoose']


class Spy:
    """np.random.choice that remembers the p it was given"""

    def __init__(self):
        self.p = None
        self.real = np.random.choice

    def __call__(self, a, p=None, **kw):
        self.p = np.array(p, dtype=np.float64)
        return self.real(a, p=p, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('HOPE_REFERENCE'), required=not os.environ.get('HOPE_REFERENCE'))
    ap.add_argument('--choices', type=int, default=40000)
    args = ap.parse_args()
    SceneChoose, DlpCaseChoose = load_choosers(args.reference)
    from hope_amd import curriculum as cu
    rng = np.random.default_rng(20240917)
    np.random.seed(7)
    spy = Spy()
    np.random.choice = spy

    # ---- _choose_case_worst_perform: the p vector for seeded success histories ----
    # (rates: mixed, all above the targets, all failing, short histories, one type far behind)
    type_rates = [(0.6, 0.4, 0.2, 0.7), (0.99, 0.99, 0.99, 1.0), (0.0, 0.0, 0.0, 0.0), (0.9, 0.5, 0.93, 0.3), (0.97, 0.96, 0.1, 0.995),
                  (0.5, 0.5, 0.5, 0.5)]
    type_lens = [(400, 300, 260, 500), (250, 251, 1000, 300), (300, 300, 300, 300), (40, 3, 120, 250), (600, 600, 600, 600), (1, 2, 5, 9)]
    thn, ths, tp = [], [], []
    for rates, lens in zip(type_rates, type_lens):
        sc = SceneChoose()
        for t in range(4):
            sc.success_record[t] = [int(x) for x in (rng.random(lens[t]) < rates[t])]
        sc._choose_case_worst_perform()
        thn.append([min(250, lens[t]) for t in range(4)])
        ths.append([int(np.sum(sc.success_record[t][-250:])) for t in range(4)])
        tp.append(spy.p.copy())

    # ---- DlpCaseChoose.choose_case: its p vector (the branch behind the 0.2 coin and the 500-episode horizon) ----
    chn, chs, cp = [], [], []
    for h in range(6):
        dc = DlpCaseChoose()
        nc = dc.dlp_case_num
        base = [0.3, 0.9, 0.0, 1.0, 0.6, 0.5][h]
        rate = np.clip(base + rng.normal(0, 0.25, nc), 0, 1)
        lens = rng.integers(0, 25, nc)
        lens[:6] = [0, 1, 1, 2, 10, 11]                      # cases with <= 1 record, and both sides of the 10-record window
        if h == 3:
            lens[:] = np.maximum(lens, 2)                    # every case recorded, every recent record a success
            lens[:3] = [0, 1, 1]
        for c in range(nc):
            for x in (rng.random(lens[c]) < rate[c]):
                dc.update_success_record(int(x), c)
        while len(dc.case_record) < dc.horizon:              # pad beyond the horizon with one busy case
            dc.update_success_record(int(rng.random() < 0.5), nc - 1)
        spy.p = None
        for _ in range(200):                                 # the 0.2 coin: repeat until the weighted branch ran
            dc.choose_case()
            if spy.p is not None:
                break
        assert spy.p is not None
        n = [len(dc.case_success_rate[str(c)]) for c in range(nc)]
        chn.append([min(10, k) for k in n])
        chs.append([int(np.sum(dc.case_success_rate[str(c)][-10:])) for c in range(nc)])
        cp.append(spy.p.copy())

    # ---- SceneChoose.choose_case: long-run type frequencies for frozen histories ----
    freq_rates = [(0.6, 0.4, 0.2, 0.7), (0.95, 0.94, 0.3, 0.99), (0.2, 0.9, 0.9, 0.98), (0.93, 0.93, 0.88, 0.97)]
    fhn, fhs, freq = [], [], []
    margin = 0.0
    for rates in freq_rates:
        sc = SceneChoose()
        for t in range(4):
            sc.success_record[t] = [int(x) for x in (rng.random(250) < rates[t])]
        for _ in range(sc.history_horizon):                  # past the warm-up
            sc.choose_case()
        names = {v: k for k, v in sc.scene_types.items()}
        cnt = np.zeros(4)
        for _ in range(args.choices):
            cnt[names[sc.choose_case()]] += 1
        n = [250] * 4
        s = [int(np.sum(sc.success_record[t])) for t in range(4)]
        f = cnt / cnt.sum()
        q = cu.type_q(n, s)
        margin = max(margin, float(np.abs(f - q).max()))
        print('rates', rates, 'freq', np.round(f, 4), 'q', np.round(q, 4), 'max dev', np.abs(f - q).max())
        fhn.append(n); fhs.append(s); freq.append(f)

    out = os.path.join(HERE, 'curriculum.npz')
    np.savez_compressed(out, type_hist_n=np.array(thn, np.float64), type_hist_s=np.array(ths, np.float64), type_p=np.array(tp),
                        case_hist_n=np.array(chn, np.float64), case_hist_s=np.array(chs, np.float64), case_p=np.array(cp),
                        freq_hist_n=np.array(fhn, np.float64), freq_hist_s=np.array(fhs, np.float64), freq=np.array(freq),
                        freq_choices=np.int64(args.choices), freq_margin=np.float64(margin))
    print('wrote', out, 'freq_margin', margin)


if __name__ == '__main__':
    main()
