"""CPU: the workspace size queries of the matcher, the tokeniser and the samplers answer what they answered before their layouts were
written once (one layout function per workspace, read by the query and by the entry point), every entry point refuses a workspace one
byte short of its query's answer before it touches a device, and the new query is exported, bound and declared.

The size queries are plain host functions and the library loads without a GPU.  The refused calls dereference none of their device
pointers: they get addresses inside one small host buffer.  No call here passes the full size."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from linetr_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (function, arguments, bytes).  Made by calling the library as it was BEFORE the layouts were single-sourced with these arguments and
# printing the answers; the table is regenerated on purpose when a layout changes on purpose, never to make a failing row pass.  The
# layout arithmetic is not restated here: that would be one more copy to keep in step.
SIZES = [
    ("linetr_match_workspace_bytes", (1, 0, 0, 0), 768),
    ("linetr_match_workspace_bytes", (1, 1500, 1050, 65), 9216),
    ("linetr_match_workspace_bytes", (1, 1023, 0, 64), 6912),
    ("linetr_match_workspace_bytes", (2, 3088, 0, 146), 18432),
    ("linetr_match_workspace_bytes", (8, 32760, 0, 1016), 173312),
    ("linetr_match_workspace_bytes", (9, 270, 0, 63), 4608),
    ("linetr_match_workspace_bytes", (64, 67108800, 0, 131072), 305143552),
    ("linetr_match_workspace_bytes", (1, 16785409, 0, 8194), 75731968),
    ("linetr_match_workspace_bytes", (1, 17425, 0, 1042), 104192),
    ("linetr_match_distmat_workspace_bytes", (0, 0), 768),
    ("linetr_match_distmat_workspace_bytes", (1, 1), 1280),
    ("linetr_match_distmat_workspace_bytes", (17, 64), 6912),
    ("linetr_match_distmat_workspace_bytes", (63, 65), 20736),
    ("linetr_match_distmat_workspace_bytes", (64, 1023), 307968),
    ("linetr_match_distmat_workspace_bytes", (1024, 1025), 4748544),
    ("linetr_match_distmat_workspace_bytes", (4097, 1), 68864),
    ("linetr_match_distmat_workspace_bytes", (-1, 5), 768),
    ("linetr_match_distmat_f64_workspace_bytes", (0, 0), 512),
    ("linetr_match_distmat_f64_workspace_bytes", (1, 1), 1024),
    ("linetr_match_distmat_f64_workspace_bytes", (5, 64), 1024),
    ("linetr_match_distmat_f64_workspace_bytes", (63, 65), 1536),
    ("linetr_match_distmat_f64_workspace_bytes", (1025, 1024), 17152),
    ("linetr_match_distmat_f64_workspace_bytes", (4097, 4097), 66560),
    ("linetr_match_distmat_f64_workspace_bytes", (5, -1), 1024),
    ("linetr_pool_distmat_workspace_bytes", (0, 0), 512),
    ("linetr_pool_distmat_workspace_bytes", (1, 1), 512),
    ("linetr_pool_distmat_workspace_bytes", (64, 65), 3584),
    ("linetr_pool_distmat_workspace_bytes", (1023, 1025), 541696),
    ("linetr_pool_distmat_workspace_bytes", (4097, 63), 163328),
    ("linetr_pool_distmat_dense_workspace_bytes", (0, 0, 0, 0), 2048),
    ("linetr_pool_distmat_dense_workspace_bytes", (1, 1, 1, 1), 2048),
    ("linetr_pool_distmat_dense_workspace_bytes", (63, 64, 65, 1023), 270592),
    ("linetr_pool_distmat_dense_workspace_bytes", (30, 40, 35, 50), 8960),
    ("linetr_pool_distmat_dense_workspace_bytes", (1024, 1025, 1025, 4097), 17365248),
    ("linetr_pool_distmat_dense_workspace_bytes", (65, 64, 5, 4), 3584),
    ("linetr_tokenize_workspace_bytes", (1, 64, 96, 1), 98816),
    ("linetr_tokenize_workspace_bytes", (2, 64, 96, 37), 197120),
    ("linetr_tokenize_workspace_bytes", (1, 480, 640, 1023), 4919552),
    ("linetr_tokenize_workspace_bytes", (8, 1024, 1024, 4097), 134234624),
    ("linetr_tokenize_workspace_bytes", (9, 65, 63, 0), 516608),
    ("linetr_tokenize_workspace_bytes", (64, 8, 8, 64), 66048),
    ("linetr_sample_descriptors_workspace_bytes", (4, 8, 0), 32768),
    ("linetr_sample_descriptors_workspace_bytes", (4, 8, 1), 0),
    ("linetr_sample_descriptors_workspace_bytes", (63, 65, 0), 4193280),
    ("linetr_sample_descriptors_workspace_bytes", (1, 1, 0), 1024),
    ("linetr_sample_descriptors_workspace_bytes", (1025, 1023, 0), 1073740800),
    ("linetr_point_descriptors_workspace_bytes", (1, 4, 8, 0), 32768),
    ("linetr_point_descriptors_workspace_bytes", (1, 4, 8, 1), 0),
    ("linetr_point_descriptors_workspace_bytes", (9, 63, 65, 0), 37739520),
    ("linetr_point_descriptors_workspace_bytes", (64, 60, 80, 0), 314572800),
    ("linetr_point_descriptors_workspace_bytes", (0, 4, 8, 0), 0),
    ("linetr_point_descriptors_workspace_bytes", (-1, 4, 8, 0), 0),
]
# linetr_pair_tail_output_bytes: (np0, np1, k0, k1), bytes, the four offsets.  Same origin.
TAIL_OUTPUT = [
    ((33, 31, 30, 35), 8960, (0, 4096, 4352, 8704)),
    ((0, 0, 30, 35), 4608, (0, 0, 0, 4352)),
    ((33, 31, 0, 0), 4352, (0, 4096, 4352, 4352)),
    ((1, 1, 1, 1), 1024, (0, 256, 512, 768)),
    ((1025, 1023, 64, 65), 4215552, (0, 4194304, 4198656, 4215296)),
    ((4097, 4097, 1024, 1025), 71361024, (0, 67141888, 67158528, 71356928)),
]
# linetr_pair_tail_workspace_bytes: (np0, np1, n0, k0, n1, k1), what the library answered while the point matcher's part was a guess
# with 2048 bytes of slack.  The answer may only have shrunk, by less than that slack plus one alignment step.
TAIL_WORKSPACE = [
    ((33, 31, 40, 30, 50, 35), 95488),
    ((33, 31, 40, 30, 1025, 600), 352256),
    ((0, 0, 40, 30, 50, 35), 16384),
    ((33, 31, 0, 0, 0, 0), 79360),
    ((1, 64, 0, 0, 0, 0), 72448),
    ((1024, 1025, 1023, 63, 4097, 1025), 30230528),
    ((0, 0, 0, 0, 0, 0), 256),
]
TAIL_SLACK = 2048 + 256
# linetr_match_points_workspace_bytes: (n0, n1), the bytes Engine.match_points allocated while it guessed the need.  An upper bound.
POINTS = [
    ((1, 1), 5128),
    ((33, 31), 74752),
    ((17, 1025), 1177416),
    ((63, 65), 155904),
    ((1024, 1024), 6875904),
    ((4097, 1023), 24249600),
]


@pytest.fixture(scope="module")
def L():
    return nat.lib()


def test_sizes_are_what_they_were(L):
    assert len(SIZES) + len(TAIL_OUTPUT) + len(TAIL_WORKSPACE) + len(POINTS) >= 60
    for name, args, want in SIZES:
        assert getattr(L, name)(*args) == want, (name, args)
    for args, want, want_offs in TAIL_OUTPUT:
        offs = (C.c_int64 * 4)()
        assert L.linetr_pair_tail_output_bytes(*args, offs) == want and tuple(offs) == want_offs, args
        assert L.linetr_pair_tail_output_bytes(*args, None) == want, args


def test_pair_tail_workspace_only_shrinks(L):
    for args, before in TAIL_WORKSPACE:
        got = L.linetr_pair_tail_workspace_bytes(*args)
        assert before - TAIL_SLACK < got <= before, (args, got, before)
        if args[0] == 0 or args[1] == 0:                    # no point branch: nothing was guessed
            assert got == before, args


def test_match_points_query_is_aligned_covers_its_parts_and_grows_no_allocation(L):
    for (n0, n1), before in POINTS:
        got = L.linetr_match_points_workspace_bytes(n0, n1)
        # the two row-major copies of 256 floats per point and the generic matcher's workspace are the least it can hold
        floor = 1024 * (n0 + n1) + L.linetr_match_workspace_bytes(1, n0 * n1, 0, n0 + n1)
        assert got % 256 == 0 and floor <= got <= before, ((n0, n1), floor, got, before)
    for n0, n1 in ((-1, 5), (5, -1), (-3, -3)):             # negative counts clamp to 0, as the neighbouring queries do
        assert L.linetr_match_points_workspace_bytes(n0, n1) == L.linetr_match_points_workspace_bytes(max(n0, 0), max(n1, 0))


def _short_calls(L):
    """(name, call) per entry point: the call with h = NULL, dummy pointers and a workspace ONE byte below the query's answer"""
    buf = np.zeros(8192, np.uint8)
    p = (buf.ctypes.data + 255) // 256 * 256                # 256-aligned, at least 7936 bytes of the buffer behind it
    q = [p + 256 * i for i in range(16)]
    zero = np.zeros(1, np.int64)
    dims = np.array([[40, 30, 50, 35]], np.int32)
    z, d = nat.np_ptr(zero), nat.np_ptr(dims)
    need_match = L.linetr_match_workspace_bytes(1, 40 * 50, 0, 30 + 35)
    tok = nat.Tokens()
    for i, k in enumerate(("klines", "length", "angles", "sublines", "pnt", "mask", "resp", "angle_sub", "desc", "score")):
        setattr(tok, k, q[i])
    out_bytes = L.linetr_pair_tail_output_bytes(33, 31, 30, 35, None)
    calls = [
        ("linetr_match", lambda: L.linetr_match(None, 1, d, q[0], z, q[1], q[2], z, q[3], 0.8, 1, q[4], z, q[5], z, q[6], need_match - 1, None)),
        ("linetr_match_gathered", lambda: L.linetr_match_gathered(None, 1, d, q[0], z, q[1], z, q[2], z, q[3], z, 0.8, 1, q[4], z, q[5], z, q[6],
                                                                  need_match - 1, None)),
        ("linetr_match_points", lambda: L.linetr_match_points(None, q[0], 33, q[1], 31, 0.8, 1, q[2], q[3], q[4],
                                                              L.linetr_match_points_workspace_bytes(33, 31) - 1, None)),
        ("linetr_pair_tail", lambda: L.linetr_pair_tail(None, q[0], 33, q[1], 31, 0.7, q[2], 40, q[3], 30, q[4], 50, q[5], 35, 0.8, 1, q[6], out_bytes,
                                                        q[7], L.linetr_pair_tail_workspace_bytes(33, 31, 40, 30, 50, 35) - 1, None)),
        ("linetr_match_distmat", lambda: L.linetr_match_distmat(None, q[0], 17, 64, 0.8, 1, q[1], q[2],
                                                                L.linetr_match_distmat_workspace_bytes(17, 64) - 1, None)),
        ("linetr_match_distmat_f64", lambda: L.linetr_match_distmat_f64(None, q[0], 5, 64, 0.8, 1, q[1], q[2],
                                                                        L.linetr_match_distmat_f64_workspace_bytes(5, 64) - 1, None)),
        ("linetr_tokenize", lambda: L.linetr_tokenize(None, q[10], 3, 5, 8.0, 3, q[11], q[12], 2, 64, 96, 0, 0, 0, 0, tok, q[13], q[14],
                                                      L.linetr_tokenize_workspace_bytes(2, 64, 96, 5) - 1, None)),
        ("linetr_sample_descriptors", lambda: L.linetr_sample_descriptors(None, q[0], 4, q[1], 4, 8, 0, 0, q[2], q[3],
                                                                          L.linetr_sample_descriptors_workspace_bytes(4, 8, 0) - 1, None)),
        ("linetr_point_descriptors", lambda: L.linetr_point_descriptors(None, q[0], q[1], 1, 4, q[2], 4, 8, 0, 0, q[3], q[4],
                                                                        L.linetr_point_descriptors_workspace_bytes(1, 4, 8, 0) - 1, None)),
    ]
    return buf, calls


def test_one_byte_short_is_refused_before_anything_else_happens(L):
    buf, calls = _short_calls(L)
    assert len(calls) == 9
    for name, call in calls:
        assert call() == nat.E_WORKSPACE, (name, L.linetr_last_error().decode())
        assert "workspace too small" in L.linetr_last_error().decode(), name
    assert not buf.any()


def test_new_query_is_bound_declared_and_exported(L):
    name = "linetr_match_points_workspace_bytes"
    header = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    decl, entry = re.search(r"\b%s\(" % name, header), re.search(r"\blinetr_match_points\(", header)
    assert name in nat.ABI and decl and entry and decl.start() < entry.start()
    names = list(nat.ABI)
    assert names.index(name) + 1 == names.index("linetr_match_points")          # the binding keeps the header's order
    assert "#define LINETR_ABI_VERSION 6" in header
    assert hasattr(L, name)
