"""CPU-side tests (-m "not gpu"): host tables, scene sources, the C-ABI library's exported symbols,
wrapper arithmetic, path sampler.  No kernel is launched here."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_tables_bit_identical_to_reference(gold):
    """hope_amd.tables restates ActionMask.__init__ with numpy: on the numpy build that produced the
    fixtures the tables carry the reference's own rounding (sha256 of the 4 MB dist_star)."""
    from hope_amd import tables as T
    g = gold('constants.npz')
    t = T.all_tables()
    assert np.array_equal(t['actions'], g['discrete_actions'])
    assert np.abs(T.swept_boxes() - g['vehicle_boxes']).max() < 1e-12
    assert np.abs(T.dist_star_coarse() - g['dist_star_coarse']).max() < 1e-12
    assert np.abs(t['dist_star'][::7] - g['dist_star_every7']).max() < 1e-12
    assert abs(t['dist_star'].sum() - float(g['dist_star_sum'])) < 1e-6
    assert np.abs(t['beam_ab'][:, 0] - g['beam_a']).max() < 1e-15 and np.abs(t['beam_ab'][:, 1] - g['beam_b']).max() < 1e-15
    if np.array_equal(T.dist_star_coarse(), g['dist_star_coarse']):        # same numpy SIMD path as the fixture
        assert hashlib.sha256(t['dist_star'].tobytes()).hexdigest() == str(g['dist_star_sha256'])
    assert t['hull_base'][0] == 3.76 and abs(t['hull_base'][30] - 0.97) < 1e-15 and abs(t['hull_base'][60] - 0.93) < 1e-15


def test_tables_agree_with_oracle():
    from hope_amd import tables as T
    from oracle import oracle as O
    t, o = T.all_tables(), O.tables()
    assert np.array_equal(t['actions'], o['actions'])
    assert np.abs(t['dist_star'] - o['dist_star']).max() < 1e-12
    assert np.abs(t['hull_base'] - o['hull_base']).max() < 1e-14
    assert np.abs(t['beam_ab'][:, 0] - o['beam_a']).max() < 1e-15


def test_library_exports_every_declared_symbol():
    """the C-ABI library loads (no GPU needed for dlopen) and exports exactly what include/hope_env.h declares."""
    from hope_amd import build_extension, lib_path
    from hope_amd import _lib
    build_extension()
    hdr = open(os.path.join(ROOT, 'include', 'hope_env.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(hope_[a-z_0-9]+)\s*\(', hdr))
    declared = {d for d in declared if not d.endswith('_t')}
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = ctypes.CDLL(lib_path())
    for name in declared:
        assert hasattr(lib, name), name
    L = _lib.load_library()
    assert L.hope_abi_version() == _lib.ABI_VERSION == 8


def _header(name=os.path.join('include', 'hope_env.h'), keep_comments=False):
    text = open(os.path.join(ROOT, name)).read()
    return text if keep_comments else re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def _c_number(text):
    """the value of a numeric macro / constexpr body: literals, parentheses, shifts, a minus sign, an unsigned suffix"""
    text = re.sub(r'\b(0[xX][0-9a-fA-F]+|\d+)[uU]\b', r'\1', text.strip())
    assert re.fullmatch(r'[0-9a-fA-FxX.()<\- ]+', text), text
    return eval(text, {'__builtins__': {}})


def test_prototype_table_mirrors_the_header():
    """_lib.PROTOTYPES against include/hope_env.h: every prototype's return type, parameter count and the kind of every parameter
    (pointer, int / int32_t, uint32_t, int64_t, uint64_t, double, size_t -- compared by size and signedness, not by ctypes identity)."""
    from hope_amd import _lib
    hdr = re.sub(r'^\s*#.*$', '', _header(), flags=re.M)
    protos = re.findall(r'([\w \t\*]+?)\b(hope_\w+)\s*\(([^;{]*?)\)\s*;', hdr)
    assert len(protos) >= 98 and len({p[1] for p in protos}) == len(protos), len(protos)
    assert {p[1] for p in protos} == set(_lib.EXPORTS)
    ints = {'int': (4, True), 'int32_t': (4, True), 'uint32_t': (4, False), 'int64_t': (8, True), 'uint64_t': (8, False),
            'size_t': (ctypes.sizeof(ctypes.c_size_t), False)}

    def agrees(param, ct):
        words = param.replace('*', ' * ').split()
        if '*' in words:
            return ct in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ct, ctypes._Pointer)
        base = [w for w in words[:-1] if w != 'const']
        assert len(base) == 1 and (base[0] in ints or base[0] == 'double'), f'unknown parameter kind: {param!r}'
        if base[0] == 'double':
            return ct is ctypes.c_double
        size, signed = ints[base[0]]
        return issubclass(ct, ctypes._SimpleCData) and ct._type_ in 'iIlLqQ' and ctypes.sizeof(ct) == size and (ct(-1).value < 0) == signed

    for ret, name, params in protos:
        restype, argtypes = _lib.PROTOTYPES[name]
        ret = ' '.join(ret.replace('*', ' * ').split())
        assert (ret, restype) in (('int', ctypes.c_int), ('const char *', ctypes.c_char_p)), (name, ret, restype)
        params = [] if params.strip() == 'void' else [p.strip() for p in params.split(',')]
        assert len(params) == len(argtypes), (name, params, argtypes)
        for i, (p, ct) in enumerate(zip(params, argtypes)):
            assert agrees(p, ct), (name, i, p, ct)
    L = _lib.load_library()                                 # and the table is what the loaded functions carry
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == list(argtypes), name


def test_constants_mirror_the_header():
    """every upper-case number of _lib equals its HOPE_ define; KERNELS is the HOPE_K_ order; the constants without a public define are
    listed here, each with the internal definition it restates"""
    from hope_amd import _lib
    defines = {m.group(1): _c_number(m.group(2)) for m in re.finditer(r'^[ \t]*#define[ \t]+HOPE_(\w+)[ \t]+([^\n]+?)[ \t]*$', _header(), flags=re.M)}
    numbers = {k: v for k, v in vars(_lib).items() if k.isupper() and isinstance(v, (int, float)) and not isinstance(v, bool)}
    assert 'ABI_VERSION' in numbers and 'CURRICULUM_LIST_LEN' in numbers and len(numbers) >= 45
    private = {k for k in numbers if k not in defines}
    assert private == {'STAGE_NO_CULL', 'STAGE_ONE_SCENE', 'CHOOSE_FALLBACK', 'BUCKET_UNLABELLED'}, private
    for k in numbers.keys() - private:
        assert numbers[k] == defines[k] and type(numbers[k]) is type(defines[k]), (k, numbers[k], defines[k])
    internal = _header(os.path.join('hope_amd', 'csrc', 'hope_internal.h'))
    for k in ('STAGE_NO_CULL', 'STAGE_ONE_SCENE'):
        assert numbers[k] == _c_number(re.search(r'constexpr\s+uint32_t\s+%s\s*=\s*([^;]+);' % k, internal).group(1)), k
    for k, macro, name in (('CHOOSE_FALLBACK', 'CH_FALLBACK', 'hope_chooser_core.h'), ('BUCKET_UNLABELLED', 'CW_UNLABELLED', 'hope_curriculum_core.h')):
        text = _header(os.path.join('hope_amd', 'csrc', name))
        assert numbers[k] == _c_number(re.search(r'^[ \t]*#define[ \t]+%s[ \t]+([^\n]+?)[ \t]*$' % macro, text, flags=re.M).group(1)), k
    # the comment behind each HOPE_K_ define names the kernel
    kernels = {int(i): k for i, k in re.findall(r'#define[ \t]+HOPE_K_\w+[ \t]+(\d+)[ \t]*/\*[ \t]*(k_\w+)', _header(keep_comments=True))}
    assert len(_lib.KERNELS) == defines['N_KERNELS'] == len(kernels)
    assert list(_lib.KERNELS) == [kernels[i] for i in range(len(kernels))]


def test_structures_mirror_the_header():
    """field names, in order, of the three ctypes.Structure mirrors"""
    from hope_amd import _lib
    hdr = _header()
    for cls, struct in ((_lib.StepOut, 'hope_step_out'), (_lib.CurriculumParams, 'hope_curriculum_params'), (_lib.ObsNormState, 'hope_obsnorm_state')):
        body = re.search(r'typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;' % (struct, struct), hdr, flags=re.S).group(1)
        fields = [re.search(r'(\w+)\s*(\[[^\]]*\]\s*)*$', d.strip()).group(1) for d in re.split(r'[;,]', body) if d.strip()]      # (`double a[N], b[N];`)
        assert fields == [f[0] for f in cls._fields_], (struct, fields)


def test_environment_variables_are_the_documented_ones():
    """the library reads exactly the environment variables that include/hope_env.h documents, each by a literal name."""
    csrc = os.path.join(ROOT, 'hope_amd', 'csrc')
    src = ''.join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)))
    calls = re.findall(r'\bgetenv\s*\(([^)]*)\)', src)
    assert calls
    bad = [c for c in calls if not re.fullmatch(r'"HOPE_[A-Z0-9_]+"', c.strip())]
    assert not bad, bad                        # a name built at run time escapes this test
    read = {c.strip().strip('"') for c in calls}
    hdr = open(os.path.join(ROOT, 'include', 'hope_env.h')).read()
    block = re.search(r'/\* Environment variables read by the library.*?\*/', hdr, flags=re.S).group(0)
    documented = re.findall(r'^ \*   (HOPE_[A-Z0-9_]+)\s', block, flags=re.M)
    assert len(documented) == len(set(documented)), documented
    assert read == set(documented), read ^ set(documented)


def test_no_cpu_fallback():
    """without a HIP device the product path must fail loudly (never route through the oracle)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from hope_amd import _lib
    L = _lib.load_library()
    h = ctypes.c_void_p()
    rc = L.hope_env_create(ctypes.byref(h), 4, 16, 0, 0)
    assert rc == -2 and b'no CPU fallback' in L.hope_last_error()
    from hope_amd import ParkingBatch
    with pytest.raises(_lib.HopeError):
        ParkingBatch(4, 16)
    src = ''.join(open(os.path.join(ROOT, 'hope_amd', f)).read() for f in os.listdir(os.path.join(ROOT, 'hope_amd'))
                  if f.endswith('.py'))
    assert 'oracle' not in src.replace('never route through the oracle', '')


def test_dlp_pool_cull_rule_matches_reference_fixture(gold, dlp):
    """filter_obstacles (parking_map_dlp.py:88-101): the kept-obstacle lists recorded from the reference run."""
    from hope_amd.scenes import DlpScenePool, cull_obstacles
    pool = DlpScenePool()
    s = gold('rs_search.npz')
    for ri in range(len(s['case'])):
        v, nv = pool.obstacles(int(s['case'][ri]))
        keep = cull_obstacles(v, nv, s['bbox'][ri])
        want = s['keep'][s['keep_off'][ri]:s['keep_off'][ri + 1]]
        assert np.array_equal(keep, want), ri


def test_dlp_sample_semantics():
    from hope_amd.scenes import DlpScenePool, create_box, flip_orientation
    pool = DlpScenePool()
    assert len(pool) == 248
    rng = np.random.default_rng(1)
    for _ in range(50):
        s = pool.sample(rng=rng)
        assert 3 <= s.nvert.min() and s.nvert.max() <= 4 and 30 <= s.n_obst <= 128
        assert s.bbox[0] == np.floor(s.bbox[0]) and s.bbox[1] - s.bbox[0] >= 40
    p = np.array([3.0, 4.0, 0.7])
    q = flip_orientation(p)
    assert np.allclose(np.sort(create_box(p), axis=0), np.sort(create_box(q), axis=0))
    assert abs(q[2] - p[2] - np.pi) < 1e-15


def test_normal_generator_scenes_are_valid():
    from hope_amd.scenes import generate_scene, rings_distance, rings_intersect, create_box
    from oracle import oracle as O
    rng = np.random.default_rng(2)
    kinds = set()
    for lv in ('Normal', 'Complex', 'Extrem'):
        for _ in range(25):
            s = generate_scene(lv, rng)
            kinds.add((lv, s.case_id))
            assert not O.detect_collision(create_box(s.start), s.verts, s.nvert)
            assert not O.detect_collision(create_box(s.dest), s.verts, s.nvert)
            assert 3 <= s.n_obst <= 17 and (s.nvert == 4).all()
            d = np.hypot(*(s.start[:2] - s.dest[:2]))
            assert d < 25 and s.bbox[0] <= min(s.start[0], s.dest[0]) - 10
            # slot clearance rule of the rejection sampler
            gl, gr = rings_distance(create_box(s.dest), s.verts[1]), rings_distance(create_box(s.dest), s.verts[2])
            assert gl >= 0.1 - 1e-12 and gr >= 0.1 - 1e-12
    assert ('Extrem', 0) not in kinds and ('Normal', 0) in kinds and ('Normal', 1) in kinds
    # host geometry agrees with the oracle's GEOS-semantics predicate
    for _ in range(200):
        a = create_box((rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3, 3)))
        b = create_box((rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3, 3)))
        assert rings_intersect(a, b) == O.ring_intersects(a, b)


def test_wrapper_surface_is_built_on_kernel_outputs():
    """The wrapper's reward_shaping / action_rescale are not re-derived on the host: the arithmetic lives in
    the kernels (pinned to the reference's vectors through the oracle, tests/test_oracle_golden.py, and to the oracle
    on the GPU, tests/test_gpu_dropin.py); the module keeps the reference's class surface and the Status values."""
    import inspect
    from hope_amd import env as E
    assert [s.value for s in E.Status] == [1, 2, 3, 4, 5]
    assert not hasattr(E, 'reward_shaping') and not hasattr(E, 'action_rescale')
    sig = inspect.signature(E.CarParkingWrapper.__init__)
    assert list(sig.parameters)[1:] == ['env', 'action_func', 'reward_func', 'observation_func']     # env_wrapper.py:59-60
    assert list(E.REWARD_WEIGHT.keys()) == ['time_cost', 'rs_dist_reward', 'dist_reward', 'angle_reward', 'box_union_reward']


def test_rs_path_sampler_matches_reference_vectors(gold):
    """hope_amd.rs_path.PATH regenerates x/y/yaw from (ctypes, lengths): compare with calc_all_paths fixtures."""
    from hope_amd.rs_path import PATH, MAXC
    g = gold('reeds_shepp.npz')
    assert MAXC == float(g['maxc'])
    off = g['path_off']
    for i in range(0, 300):
        for k in range(off[i], off[i + 1]):
            n = int((g['ctypes'][k] >= 0).sum())
            p = PATH(g['lengths'][k][:n], ['SLR'[c] for c in g['ctypes'][k][:n]], g['q0'][i])
            assert len(p.x) == int(g['npts'][k]), (i, k)
            m = min(3, len(p.x))
            got = np.column_stack([p.x[-m:], p.y[-m:], p.yaw[-m:]])
            assert np.abs(got - g['last3'][k][3 - m:]).max() < 1e-9
            assert abs(p.L - g['L'][k]) < 1e-9


def test_dlp_pickle_reader_roundtrip(tmp_path, dlp):
    """a reference-format pickle (shapely-1.x LinearRing = WKB LineString bytes) is readable without shapely."""
    import pickle
    import struct
    import sys
    import types
    mod = types.ModuleType('shapely.geometry.polygon')

    class LinearRing:
        def __init__(self, c):
            self.c = np.asarray(c, dtype='<f8')

        def __getstate__(self):          # shapely 1.x: the pickled state is the WKB of a LineString
            c = np.vstack([self.c, self.c[:1]])
            return b'\x01' + struct.pack('<II', 2, len(c)) + c.tobytes()
    LinearRing.__module__ = 'shapely.geometry.polygon'
    LinearRing.__qualname__ = 'LinearRing'
    mod.LinearRing = LinearRing
    pkgs = {n: types.ModuleType(n) for n in ('shapely', 'shapely.geometry')}
    sys.modules.update(pkgs)
    sys.modules['shapely.geometry.polygon'] = mod
    try:
        rings = [LinearRing([(0, 0), (2, 0), (2, 1), (0, 1)]), LinearRing([(5, 5), (6, 5), (5.5, 7)])]
        case = ([(1.0, 2.0, 0.1), (1.5, 2.0, 0.2)], (9.0, 9.0, 1.57), rings)
        f = tmp_path / 'mini.data'
        f.write_bytes(pickle.dumps([case]))
    finally:
        for n in ('shapely', 'shapely.geometry', 'shapely.geometry.polygon'):
            sys.modules.pop(n, None)
    from hope_amd.dlp_io import pool_from_pickle
    pool = pool_from_pickle(str(f))
    v, nv = pool.obstacles(0)
    assert list(nv) == [4, 3] and np.array_equal(v[1, 3], v[1, 2]) and np.array_equal(v[0, 2], [2, 1])
    assert np.allclose(pool.dest[0], [9, 9, 1.57]) and len(pool.candidates(0)) == 2


def _dist_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    from hope_amd import dist as D
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    r, w, _ = D.init_from_env('gloo')
    lo, hi = D.shard_range(11, r, w)
    torch.manual_seed(0)
    net = torch.nn.Linear(7, 3)
    x = torch.arange(11 * 7, dtype=torch.float32).reshape(11, 7)[lo:hi] / 50
    loss = net(x).pow(2).sum() / 11           # per-rank share of a global-batch loss
    loss.backward()
    nbytes = D.allreduce_gradients(list(net.parameters()), average=False)
    n_local = hi - lo
    rec = D.gather_eval_stats(torch.full((n_local,), 2 if r == 0 else 3, dtype=torch.int32),
                              torch.arange(lo, hi, dtype=torch.int32), torch.ones(n_local), torch.zeros(n_local))
    q.put((r, lo, hi, net.weight.grad.clone().numpy(), nbytes, rec.numpy(), D.success_rate(rec)))
    dist.destroy_process_group()


def test_distributed_helpers_gloo_world2():
    """N > 1 path on CPU: scene sharding, one fused gradient bucket, eval-stat gather (gloo, world_size 2)."""
    import torch
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    (r0, lo0, hi0, g0, nb0, rec0, sr0), (r1, lo1, hi1, g1, nb1, rec1, sr1) = res
    assert (lo0, hi0, lo1, hi1) == (0, 6, 6, 11)
    torch.manual_seed(0)
    net = torch.nn.Linear(7, 3)
    x = torch.arange(11 * 7, dtype=torch.float32).reshape(11, 7) / 50
    (net(x).pow(2).sum() / 11).backward()
    assert np.allclose(g0, net.weight.grad.numpy(), rtol=1e-5) and np.allclose(g0, g1)
    assert nb0 == (7 * 3 + 3) * 4
    assert rec0.shape == (11, 4) and np.array_equal(rec0, rec1) and np.array_equal(rec0[:, 1], np.arange(11))
    assert abs(sr0 - 6 / 11) < 1e-6
