"""Programmed inputs of the optimiser block (hope_amd/csrc/hope_optim_core.h) and the rule restated in numpy float64, shared by
tests/test_optim_core.py (the host twin), tests/test_optim_glue.py (DeviceAdam and the agents on the twin) and tests/test_gpu_optim.py
(the kernel).

The rule, per element (f() = the one rounding to the entry's type; every other operation a double operation, no fused multiply-add --
numpy evaluates each operator on its own):
    m' = f( m + c1 * (g - m) )
    v' = f( b2 * v + (c2 * g) * g )
    p' = f( p - step_size * ( m' / ( sqrt(v') / bc2s + eps ) ) )
    polyak:  t' = f( (1 - tau) * t + tau * p )
with hyper = (c1, b2, c2, step_size, bc2s, eps) = (1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^t), sqrt(1 - beta2^t), eps)."""
import math

import numpy as np
import torch

NUMELS = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049)
STEPS = (1, 2, 1000, 10 ** 6)                      # at 10^6 both bias corrections are 1 to double precision
TAUS = (0.0, 1.0, 0.005, 0.1)
SENTINEL, PAD = -7.25, 8                           # the guard words either side of a buffer; PAD elements of them (a multiple of 16 bytes)


def hyper(lr=5e-6, betas=(0.9, 0.999), eps=1e-8, t=1):
    b1, b2 = float(betas[0]), float(betas[1])
    return (1.0 - b1, b2, 1.0 - b2, float(lr) / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), float(eps))


def adam_reference(p, g, m, v, hyper):
    """numpy arrays of one dtype (float32 or float64) -> (p', m', v') of that dtype"""
    c1, b2, c2, step_size, bc2s, eps = (np.float64(x) for x in hyper)
    dt = p.dtype
    with np.errstate(all='ignore'):
        gd, md, vd = g.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
        m2 = (md + c1 * (gd - md)).astype(dt)
        v2 = (b2 * vd + (c2 * gd) * gd).astype(dt)
        den = np.sqrt(v2.astype(np.float64)) / bc2s + eps
        p2 = (p.astype(np.float64) - step_size * (m2.astype(np.float64) / den)).astype(dt)
    return p2, m2, v2


def polyak_reference(t, p, tau):
    tau = np.float64(tau)
    omt = np.float64(1.0) - tau
    with np.errstate(all='ignore'):
        return (omt * t.astype(np.float64) + tau * p.astype(np.float64)).astype(t.dtype)


def words(x):
    """the bits of an array / tensor, for word-for-word comparison.  Every NaN counts as one word: IEEE 754 leaves the sign and payload
    of a NaN that an operation produces to the implementation (inf / inf is a negative quiet NaN on x86, a positive one on the GPU)."""
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    a = np.where(np.isnan(a), np.array(np.nan, a.dtype), a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def random_case(numel, seed, dtype=np.float32, first_step=False):
    """p ~ N(0, 0.1), g = randn * 10^k with k drawn per element from -8 .. 1, m and v a plausible running state (or the zeros of a
    first step)"""
    r = np.random.default_rng(seed)
    p = (r.standard_normal(numel) * 0.1).astype(dtype)
    g = (r.standard_normal(numel) * 10.0 ** r.integers(-8, 2, numel)).astype(dtype)
    if first_step:
        m, v = np.zeros(numel, dtype), np.zeros(numel, dtype)
    else:
        m = (r.standard_normal(numel) * 10.0 ** r.integers(-8, 2, numel)).astype(dtype)
        v = (r.standard_normal(numel) ** 2 * 10.0 ** r.integers(-16, 3, numel)).astype(dtype)
    return {'p': p, 'g': g, 'm': m, 'v': v}


# gradients whose products leave float32's normal range: (c2 * g) * g is 0 in float32 at 1e-30 and 1e-25, subnormal at 1e-20
SPECIAL_GRADS = (0.0, -0.0, 1e-30, -1e-30, 1e-25, -1e-25, 1e-20, -3e-21, 1e-38, 3e38, -3e38)
NONFINITE = (np.inf, -np.inf, np.nan)


def special_case(numel, seed, dtype=np.float32):
    """random_case with the gradients cycling through SPECIAL_GRADS, over a zero state in the first half and a running one behind it"""
    c = random_case(numel, seed, dtype)
    c['g'] = np.resize(np.array(SPECIAL_GRADS, np.float64), numel).astype(dtype)
    c['m'][:numel // 2] = 0
    c['v'][:numel // 2] = 0
    return c


def nonfinite_case(numel, seed, value, at, where='g', dtype=np.float32):
    """random_case with ONE element of `where` set to `value`"""
    c = random_case(numel, seed, dtype)
    c[where][at] = value
    return c


# ---- the programmed table: (name, case, hyper).  Every NUMEL random; the special and first-step cases at sizes on both sides of a
# lane's four elements and of a chunk; every step count; float64. ----
def case_table():
    table = []
    for i, n in enumerate(NUMELS):
        table.append((f'random-{n}', random_case(n, 100 + i), hyper(t=3)))
        table.append((f'first-{n}', random_case(n, 200 + i, first_step=True), hyper(t=1)))
    for i, n in enumerate((5, 257, 1025)):
        table.append((f'special-{n}', special_case(n, 300 + i), hyper(t=3)))
        for j, val in enumerate(NONFINITE):
            for where in ('g', 'p', 'm', 'v'):
                table.append((f'nonfinite-{n}-{j}-{where}', nonfinite_case(n, 400 + i, val, n // 2, where), hyper(t=3)))
    for i, t in enumerate(STEPS):
        table.append((f'step-{t}', random_case(1025, 500 + i), hyper(lr=2.5e-5, t=t)))
    for i, n in enumerate((1, 3, 257, 1025)):
        table.append((f'float64-{n}', random_case(n, 600 + i, np.float64), hyper(lr=1e-3, eps=1e-6, t=2)))
    return table


def guarded(x, device='cpu', offset=0):
    """the array x as a tensor view that starts `offset` elements past a 16-byte boundary, inside a buffer with PAD + offset sentinels
    in front of it and PAD behind -> (buffer, view)"""
    x = torch.from_numpy(np.ascontiguousarray(x))
    n = x.numel()
    buf = torch.full((PAD + offset + n + PAD + 4,), SENTINEL, dtype=x.dtype, device=device)
    shift = (-buf.data_ptr() % 16) // x.element_size()         # 0 with torch's allocators, which align whole tensors
    lead = PAD + shift + offset
    view = buf[lead:lead + n]
    view.copy_(x)
    assert (view.data_ptr() - offset * x.element_size()) % 16 == 0 and view.is_contiguous()
    return buf, view


def guards_intact(buf, view):
    lead = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    b = buf.detach().cpu()
    return bool((b[:lead] == SENTINEL).all()) and bool((b[lead + view.numel():] == SENTINEL).all()) and lead >= PAD


def torch_case(case, device='cpu', offset=0):
    """a case's arrays as guarded tensors -> ({name: view}, [(buffer, view)])"""
    views, bufs = {}, []
    for k, x in case.items():
        b, v = guarded(x, device, offset)
        views[k] = v
        bufs.append((b, v))
    return views, bufs


# ---- drivers shared by the host-twin and the kernel tests.  adam(params, grads, ms, vs, hypers, group_of) and polyak(targets,
# currents, tau) run ONE call over tensor lists on `device`. ----
def run_table(adam, device, offsets=(0,), reference=adam_reference):
    """the whole case table in as few calls as four groups to a call allow, entry i based offsets[i % len] elements past a 16-byte
    boundary.  Asserts every word of p, m, v against reference(p, g, m, v, hyper) and every guard; -> the number of calls."""
    table = case_table()
    hypers = []
    for _, _, hp in table:
        if hp not in hypers:
            hypers.append(hp)
    calls = 0
    for at in range(0, len(hypers), 4):
        hs = hypers[at:at + 4]
        rows = [(name, case, hs.index(hp)) for name, case, hp in table if hp in hs]
        views, bufs = [], []
        for i, (_, case, _) in enumerate(rows):
            v, b = torch_case(case, device, offsets[i % len(offsets)])
            views.append(v)
            bufs += b
        adam([v['p'] for v in views], [v['g'] for v in views], [v['m'] for v in views], [v['v'] for v in views], hs, [r[2] for r in rows])
        calls += 1
        for (name, case, gi), v in zip(rows, views):
            want = reference(case['p'], case['g'], case['m'], case['v'], hs[gi])
            for k, w in zip('pmv', want):
                assert np.array_equal(words(v[k]), words(w)), (name, k, int((words(v[k]) != words(w)).sum()))
            assert np.array_equal(words(v['g']), words(case['g'])), (name, 'the gradient was written')
        assert all(guards_intact(b, v) for b, v in bufs), 'a guard word was written'
    return calls


def refusals(lib_module, f32, f64):
    """every call the ABI refuses -> [(label, mode, entries, n, groups, n_groups, tau, text the message must hold)].  f32, f64: dicts
    of p, g, m, v views (two float32 entries are built from f32's halves).  mode 'adam' / 'polyak'."""
    L = lib_module
    h = f32['p'].numel() // 2
    es = 4

    def ent(src, lo, n, dtype=L.OPTIM_F32, group=0, esz=4, **over):
        e = L.OptimEntry(*(src[k].data_ptr() + lo * esz for k in 'pgmv'), n, group, dtype)
        for k, val in over.items():
            setattr(e, k, val)
        return e

    def tab(*es_):
        return (L.OptimEntry * len(es_))(*es_)
    good = lambda: [ent(f32, 0, h), ent(f32, h, h)]  # noqa: E731
    g1 = (L.OptimGroup * 1)(L.OptimGroup(*hyper(t=2)))
    out = [('null table', 'adam', None, 2, g1, 1, 0.0, 'null entry table'),
           ('null groups', 'adam', tab(*good()), 2, None, 1, 0.0, 'null group table'),
           ('n_entries 0', 'adam', tab(*good()), 0, g1, 1, 0.0, 'n_entries < 1'),
           ('n_entries -1', 'adam', tab(*good()), -1, g1, 1, 0.0, 'n_entries < 1'),
           ('n_groups 0', 'adam', tab(*good()), 2, g1, 0, 0.0, 'n_groups must be 1 .. 4'),
           ('n_groups 5', 'adam', tab(*good()), 2, (L.OptimGroup * 5)(*[L.OptimGroup(*hyper(t=2))] * 5), 5, 0.0, 'n_groups must be 1 .. 4')]
    for k in 'pgmv':
        out.append((f'null {k}', 'adam', tab(good()[0], ent(f32, h, h, **{k: None})), 2, g1, 1, 0.0, 'entry 1: null pointer'))
        out.append((f'misaligned {k}', 'adam', tab(good()[0], ent(f32, h, h, **{k: f32[k].data_ptr() + h * es + 2})), 2, g1, 1, 0.0,
                    'entry 1: a pointer is not aligned to its element'))
        out.append((f'misaligned float64 {k}', 'adam', tab(ent(f64, 0, 1, L.OPTIM_F64, 0, 8, **{k: f64[k].data_ptr() + 4})), 1, g1, 1, 0.0,
                    'entry 0: a pointer is not aligned to its element'))
    out += [('numel 0', 'adam', tab(good()[0], ent(f32, h, 0)), 2, g1, 1, 0.0, 'entry 1: numel < 1'),
            ('numel -3', 'adam', tab(ent(f32, 0, -3), good()[1]), 2, g1, 1, 0.0, 'entry 0: numel < 1'),
            ('one entry past 2^31', 'adam', tab(good()[0], ent(f32, h, 2 ** 31 + 1)), 2, g1, 1, 0.0, 'entry 1: more than 2^31 elements'),
            ('a total past 2^31', 'adam', tab(ent(f32, 0, 2 ** 30), ent(f32, h, 2 ** 30 + 1)), 2, g1, 1, 0.0, 'entry 1: more than 2^31 elements'),
            ('group -1', 'adam', tab(good()[0], ent(f32, h, h, group=-1)), 2, g1, 1, 0.0, 'entry 1: group index out of range'),
            ('group 1 of 1', 'adam', tab(ent(f32, 0, h, group=1), good()[1]), 2, g1, 1, 0.0, 'entry 0: group index out of range'),
            ('dtype 2', 'adam', tab(good()[0], ent(f32, h, h, dtype=2)), 2, g1, 1, 0.0, 'entry 1: dtype is neither'),
            ('dtype -1', 'adam', tab(good()[0], ent(f32, h, h, dtype=-1)), 2, g1, 1, 0.0, 'entry 1: dtype is neither')]
    for fi, field in enumerate(('c1', 'b2', 'c2', 'step_size', 'bc2s', 'eps')):
        for bad in (float('nan'), float('inf'), float('-inf')):
            hp = list(hyper(t=2))
            hp[fi] = bad
            out.append((f'{field} {bad}', 'adam', tab(*good()), 2, (L.OptimGroup * 2)(L.OptimGroup(*hyper(t=2)), L.OptimGroup(*hp)), 2, 0.0,
                        'group 1: a hyper-parameter is not finite'))
    for field, bad, text in (('eps', -1e-8, 'group 0: eps < 0'), ('bc2s', 0.0, 'group 0: bc2s <= 0'), ('bc2s', -0.5, 'group 0: bc2s <= 0')):
        hp = dict(zip(('c1', 'b2', 'c2', 'step_size', 'bc2s', 'eps'), hyper(t=2)))
        hp[field] = bad
        out.append((f'{field} {bad}', 'adam', tab(*good()), 2, (L.OptimGroup * 1)(L.OptimGroup(**hp)), 1, 0.0, text))
    for tau in (-0.1, 1.0000001, float('nan'), float('inf')):
        out.append((f'tau {tau}', 'polyak', tab(*good()), 2, None, 0, tau, 'tau must be in [0, 1]'))
    out += [('polyak null table', 'polyak', None, 1, None, 0, 0.5, 'null entry table'),
            ('polyak n_entries 0', 'polyak', tab(*good()), 0, None, 0, 0.5, 'n_entries < 1'),
            ('polyak null target', 'polyak', tab(good()[0], ent(f32, h, h, p=None)), 2, None, 0, 0.5, 'entry 1: null pointer'),
            ('polyak null current', 'polyak', tab(ent(f32, 0, h, g=None), good()[1]), 2, None, 0, 0.5, 'entry 0: null pointer'),
            ('polyak misaligned', 'polyak', tab(good()[0], ent(f32, h, h, g=f32['g'].data_ptr() + h * es + 1)), 2, None, 0, 0.5,
             'entry 1: a pointer is not aligned to its element'),
            ('polyak numel 0', 'polyak', tab(ent(f32, 0, 0)), 1, None, 0, 0.5, 'entry 0: numel < 1'),
            ('polyak dtype 7', 'polyak', tab(ent(f32, 0, h, dtype=7)), 1, None, 0, 0.5, 'entry 0: dtype is neither')]
    return out
