"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports exactly what
include/mvp_hip.h declares; the host mirror refuses CPU tensors (no fallback)."""
import os
import re

import pytest
import torch

from tests.conftest import ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'mvp_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(mvp_[a-z0-9_]+)\s*\(', text)))


def test_header_symbols_are_exported():
    from mvpnet_amd import _lib
    lib = _lib.lib()
    names = declared_symbols()
    assert len(names) >= 26
    for name in names:
        assert hasattr(lib, name), 'libmvp_hip.so does not export ' + name
    assert sorted(_lib.EXPORTS) == names, 'python signature table and header disagree'
    assert b'gfx950' in lib.mvp_version()
    assert lib.mvp_strerror(-1).startswith(b'invalid argument')


def test_signature_table_matches_the_header_argument_counts():
    """Every ctypes signature in mvpnet_amd/_lib.py has as many entries as the header's prototype has parameters (stream included):
    ctypes accepts extra positional arguments silently, so a short table would go unnoticed."""
    import re
    from mvpnet_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mvp_hip.h')).read(), flags=re.S)
    for name, sig in _lib._SIGNATURES.items():
        m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', text, flags=re.S)
        assert m, name
        n = len([a for a in m.group(1).split(',') if a.strip() not in ('', 'void')])   # `(void)`: no parameters
        assert n == len(sig), (name, n, len(sig))


def test_argument_errors_do_not_launch():
    """Precondition failures return MVP_E* before any HIP call (safe without a GPU)."""
    import ctypes
    from mvpnet_amd import _lib
    lib = _lib.lib()
    dummy = ctypes.c_void_p(16)
    assert lib.mvp_fps_f32(None, 1, 8, 3, 4, dummy, None) == -3                    # MVP_ENULL
    assert lib.mvp_fps_f32(dummy, 1, 8, 3, 9, dummy, None) == -1                   # N >= M   (fps_kernel.cu:156)
    assert lib.mvp_fps_f32(dummy, 1, 8, 4, 4, dummy, None) == -1                   # D in {2,3}
    assert lib.mvp_knn_distance_f32(dummy, dummy, 1, 4, 8, 5, dummy, dummy, None) == -2   # k must be 3 (:171)
    assert lib.mvp_knn_distance_f32(dummy, dummy, 1, 4, 2, 3, dummy, dummy, None) == -1   # N2 >= k
    assert lib.mvp_pixel_knn_bruteforce_f32(dummy, dummy, dummy, 1, 8, 8, 9, dummy, None, None) == -1


def test_set_abstraction_level_limits_are_refused_before_any_launch():
    """The fused set-abstraction kernels do 32-bit ball and row-offset arithmetic: the three entry points refuse B*M > 2^31 - 16, N or
    M > INT_MAX and N * max(C1, 3) >= 2^32 with MVP_EUNSUPPORTED, after the null and size checks and before any HIP call (safe without a
    GPU: every call here is over a limit or invalid)."""
    import ctypes
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)
    C1, C2, C3 = 64, 64, 128
    # a split-bf16 precision, set here: without one the entry points answer MVP_EUNSUPPORTED before they look at the limits
    old = lib.mvp_get_mlp_precision(), lib.mvp_get_mlp_precision_backward()
    assert lib.mvp_set_mlp_precision(6, _lib.mlp_min_width()) == 0 and lib.mvp_set_mlp_precision_backward(3) == 0

    def level(B, N, M, K, xyz):   # zf, xyz, centre, index, wxyz, B, N, M, K, C1, bn1 x 4, W2, C2, bn2 x 4, W3, C3
        return (d, xyz, d, d, d, B, N, M, K, C1, d, d, d, d, d, C2, d, d, d, d, d, C3)

    def inference(*lv):
        return lib.mvp_sa_fused_forward_f32(*level(*lv), d, d, d, d, d, None, None)

    def forward(stage):
        return lambda *lv: lib.mvp_sa_train_forward_f32(stage, *level(*lv), d, 1e-5, 0.1, d, d, None, None, None, d, d, d, d, None)

    def backward(layer):
        own = (None, d, d, d, None) if layer == 3 else (d, None, None, None, d)   # G, pool_dout, pool_out, pool_arg, tsum
        return lambda *lv: lib.mvp_sa_train_backward_f32(layer, *level(*lv), d, d, d, d, None, None, 1, *own[:4], d, 64, d, d, own[4], None)

    try:
        for entry in (inference, forward(2), forward(3), backward(2), backward(3)):
            assert entry(2 ** 20, 1000, 2 ** 11, 32, d) == -2    # B * M = 2^31
            assert entry(2, 2 ** 31, 10, 32, d) == -2            # N
            assert entry(2, 2 ** 26, 10, 32, d) == -2            # N * C1 = 2^32
            assert entry(2, 1000, 10, 32, None) == -3            # MVP_ENULL comes first, as before
            assert entry(2, 1000, 10, 0, d) == -1                # ... and so does MVP_EINVAL
            assert entry(2 ** 20, 1000, 2 ** 11, 32, None) == -3 and entry(2, 2 ** 31, 10, 0, d) == -1
            assert entry(2, 1000, 10, 0, None) == -3             # a null pointer outranks an invalid size
    finally:
        assert lib.mvp_set_mlp_precision(old[0], _lib.mlp_min_width()) == 0 and lib.mvp_set_mlp_precision_backward(old[1]) == 0


@pytest.mark.parametrize('fn', ['fps', 'ball', 'knn', 'group', 'interp'])
def test_no_cpu_fallback(fn):
    import mvpnet_amd.ops as ops
    x = torch.rand(1, 3, 16)
    with pytest.raises(RuntimeError):
        if fn == 'fps':
            ops.farthest_point_sample(x, 4)
        elif fn == 'ball':
            ops.ball_query(x, x, 0.1, 4)
        elif fn == 'knn':
            ops.knn_distance(x, x, 3)
        elif fn == 'group':
            ops.group_points(x, torch.zeros(1, 2, 2, dtype=torch.long))
        else:
            ops.feature_interpolate(x, torch.zeros(1, 2, 3, dtype=torch.long), torch.rand(1, 2, 3))


def test_product_does_not_import_oracle():
    """The product package must never route through oracle/ (tier rule 3)."""
    pkg = os.path.join(ROOT, 'mvpnet_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', text, flags=re.M), f
                assert 'mvp_oracle' not in text and 'c_oracle' not in text, f


def test_thread_local_precision_scope():
    """mvp_mlp_precision_scope: a thread-local override of the contraction precision (nothing process-wide is written): another thread
    keeps seeing the process default while this one is inside a scope."""
    import threading
    from mvpnet_amd import _lib as L
    lib = L.lib()
    default = lib.mvp_get_mlp_precision()
    seen = {}
    with L.mlp_precision('fp32'):
        assert lib.mvp_get_mlp_precision() == 0
        t = threading.Thread(target=lambda: seen.setdefault('other', lib.mvp_get_mlp_precision()))
        t.start()
        t.join()
        with L.mlp_precision('bf16x3', backward='bf16x6'):
            assert lib.mvp_get_mlp_precision() == 3 and lib.mvp_get_mlp_precision_backward() == 6
        assert lib.mvp_get_mlp_precision() == 0
    assert seen['other'] == default and lib.mvp_get_mlp_precision() == default
    assert lib.mvp_mlp_precision_scope(5, -1) == -1  # MVP_EINVAL
    with L.mlp_precision('bf16', backward='bf16'):  # plain bf16 operands, one product (opt-in)
        assert lib.mvp_get_mlp_precision() == 1 and lib.mvp_get_mlp_precision_backward() == 1
    assert lib.mvp_get_mlp_precision() == default


def test_derived_types_of_pinned_prototypes():
    """The tables mvpnet_amd/_lib.py derives from the header against hand-written argtypes AND restype of prototypes that between them use
    every C type of the header: a c_int for an int64_t, a c_float for a double or a status restype on a size_t return shows here."""
    from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p
    from mvpnet_amd import _lib as L
    p, i64 = c_void_p, c_int64
    pinned = {
        'mvp_adam_step_f32': ([p] * 5 + [i64] + [c_double] * 6 + [p], c_int),
        'mvp_sample_chunks_f32': ([p] * 6 + [i64] * 6 + [c_double] * 5 + [c_int, c_uint64] + [p] * 9 + [i64, p], c_int),
        'mvp_bn_rows_forward_dropout_f32': ([p, p, p, i64, i64, c_int, c_float, c_float, c_int] + [p] * 7 + [c_float, c_uint64, p], c_int),
        'mvp_lift_f32': ([p, c_int] + [p] * 6 + [i64] * 7 + [p] * 7, c_int),
        'mvp_pn2_plan_f32': ([p, i64, i64, i64, p, p, p, p, c_int, c_int, c_float, p, i64, p, p, p], c_int),
        'mvp_prepare_frames_workspace': ([i64], c_size_t),
        'mvp_lift_workspace_bytes': ([i64] * 5, c_int64),
        'mvp_version': ([], c_char_p),
        'mvp_strerror': ([c_int], c_char_p),
    }
    for name, (argtypes, restype) in pinned.items():
        assert L._SIGNATURES[name] == argtypes, name
        assert L._RESTYPES[name] is restype, name
    assert set(L._RESTYPES) == set(L._SIGNATURES) and L.EXPORTS == sorted(L._SIGNATURES)


def test_derived_types_are_applied_to_every_function():
    """lib() sets argtypes and restype of EVERY entry point, the ones that return no status or take no stream included."""
    from mvpnet_amd import _lib as L
    lib = L.lib()
    assert len(L._SIGNATURES) == len(declared_symbols())
    for name in L._SIGNATURES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == L._SIGNATURES[name], name
        assert fn.restype is L._RESTYPES[name], name


def test_header_parser_is_strict():
    import ctypes
    from mvpnet_amd import _lib as L
    with pytest.raises(RuntimeError, match='mvp_bad_f32'):      # a scalar type outside the closed map names its prototype
        L._parse_header('int mvp_ok(int a);\nint mvp_bad_f32(const float* x, unsigned n, mvp_stream_t stream);')
    with pytest.raises(RuntimeError, match='mvp_bad_f32'):
        L._parse_header('uint8_t mvp_bad_f32(void);')
    with pytest.raises(RuntimeError, match='mvp_unnamed'):      # a parameter that does not split into type and name
        L._parse_header('int mvp_unnamed(int64_t, float* out);')
    with pytest.raises(RuntimeError, match='mvp_unnamed'):
        L._parse_header('int mvp_unnamed(int64_t n, float* const);')
    with pytest.raises(RuntimeError, match='struct'):           # a statement that is no prototype
        L._parse_header('struct mvp_s { int a; };')
    with pytest.raises(RuntimeError, match='mvp_twice'):
        L._parse_header('int mvp_twice(int a);\nint mvp_twice(int64_t a);')
    sig, res, limits = L._parse_header(
        '/* int mvp_x(int a); */\n'
        '// int mvp_y(int a);\n'
        '#define MVP_A_MAX_B 12   /* a limit */\n'
        '#define MVP_ENEG (-7)\n'
        '#define MVP_WORDS(C) (4 + (C))\n'
        '#define MVP_RATIO 0.5\n'
        '#define MVP_GUARD_H_\n'
        'typedef void* mvp_stream_t;\n'
        'int64_t mvp_three_lines_f32(const float* x,   /* mvp_z(1); */\n'
        '                            double scale, uint64_t seed,\n'
        '                            float *const *outs, mvp_stream_t stream);\n'
        'size_t mvp_nothing(void);\n')
    assert sig == {'mvp_three_lines_f32': [ctypes.c_void_p, ctypes.c_double, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p], 'mvp_nothing': []}
    assert res == {'mvp_three_lines_f32': ctypes.c_int64, 'mvp_nothing': ctypes.c_size_t}
    assert limits == {'MVP_A_MAX_B': 12, 'MVP_ENEG': -7}


def test_limits_come_from_the_header():
    from mvpnet_amd import _lib as L
    from mvpnet_amd import metric
    from mvpnet_amd.ops import chunker, ensemble, frame_eval, overlap, sample, scene_sample
    expected = {'MVP_OVERLAP_MAX_BASE': 4096, 'MVP_SAMPLE_MAX_PTS': 8192, 'MVP_SAMPLE_MAX_TRIES': 32, 'MVP_SAMPLE_MAX_CHUNKS': 65535,
                'MVP_SAMPLE_SCENE_MAX_PTS': 65536, 'MVP_CHUNKER_MAX_WINDOWS': 65535, 'MVP_PACK_CLOUD_MAX_CHANNELS': 8,
                'MVP_SEG_METER_MAX_WINDOW': 64, 'MVP_ENSEMBLE_MAX_MODELS': 8, 'MVP_CONFUSION_MAX_CLASSES': 32768, 'MVP_HISTOGRAM_MAX_BINS': 65536}
    assert {k: v for k, v in L.LIMITS.items() if '_MAX_' in k} == expected
    assert (L.LIMITS['MVP_OK'], L.LIMITS['MVP_EINVAL'], L.LIMITS['MVP_EUNSUPPORTED'], L.LIMITS['MVP_ENULL']) == (0, -1, -2, -3)
    constants = {'MVP_OVERLAP_MAX_BASE': overlap.MAX_BASE_POINTS, 'MVP_SAMPLE_MAX_PTS': sample.MAX_NB_PTS, 'MVP_SAMPLE_MAX_TRIES': sample.MAX_TRIES,
                 'MVP_SAMPLE_MAX_CHUNKS': sample.MAX_CHUNKS, 'MVP_SAMPLE_SCENE_MAX_PTS': scene_sample.MAX_SCENE_NB_PTS,
                 'MVP_CHUNKER_MAX_WINDOWS': chunker.MAX_WINDOWS, 'MVP_PACK_CLOUD_MAX_CHANNELS': chunker.MAX_CLOUD_CHANNELS,
                 'MVP_SEG_METER_MAX_WINDOW': metric.MAX_WINDOW, 'MVP_ENSEMBLE_MAX_MODELS': ensemble.MAX_MODELS,
                 'MVP_CONFUSION_MAX_CLASSES': ensemble.MAX_CONFUSION_CLASSES, 'MVP_HISTOGRAM_MAX_BINS': frame_eval.MAX_BINS}
    assert constants == expected and chunker.MAX_BASE_POINTS == expected['MVP_OVERLAP_MAX_BASE']


def test_min_width_is_read_from_the_library():
    """mvp_set_mlp_precision called directly, past the Python setter: mlp_min_width() follows (it routes layers between kernels)."""
    from mvpnet_amd import _lib as L
    lib = L.lib()
    terms, width = lib.mvp_get_mlp_precision(), L.mlp_min_width()
    try:
        assert lib.mvp_set_mlp_precision(terms, 48) == 0
        assert L.mlp_min_width() == 48
    finally:
        assert lib.mvp_set_mlp_precision(terms, width) == 0
    assert L.mlp_min_width() == width
