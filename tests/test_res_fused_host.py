"""Host tests (no GPU) of the weight packing of a 1x1 residual projection that its block's second conv evaluates itself
(cld_debug_pack_res_proj; wino1d_edge.hip reads it as ResProj::wfrag)."""
import ctypes as C

import numpy as np
import pytest

from cld_amd import _lib

# (c_out, c_in) of the projections of residual blocks 2, 4 and 8 (CLD_WINO1D_RES_INSTANCES)
SHAPES = [(128, 64), (256, 128), (128, 512)]


def _pack(W):
    lib = _lib.load()
    co, ci = W.shape
    n = lib.cld_debug_pack_res_proj(None, co, ci, None, 0)
    assert n > 0
    out = np.full(n + 8, np.float32(7.0))                        # a canary behind the buffer
    fp = C.POINTER(C.c_float)
    got = lib.cld_debug_pack_res_proj(C.cast(W.ctypes.data_as(fp), C.c_void_p), co, ci, C.cast(out.ctypes.data_as(fp), C.c_void_p), n)
    assert got == n
    assert (out[n:] == 7.0).all()
    return out[:n]


@pytest.mark.parametrize("co,ci", SHAPES)
def test_packed_projection_unpacks_to_w_and_covers_every_offset_of_the_kernel(co, ci):
    rng = np.random.default_rng(co * 1000 + ci)
    W = rng.standard_normal((co, ci)).astype(np.float32)
    frag = _pack(W)
    nch, ntn = ci // 16, co // 16
    # unpack: plane c, tile nt, lane (i16 = lane & 15, kk = lane >> 4), element e = W[16 nt + i16][16 c + 4 kk + e] -- the A operand of
    # k-step e of v_mfma_f32_16x16x4_f32 for the rows whose B operand is channel 4 kk + e of the chunk
    planes = frag[:nch * ntn * 256].reshape(nch, ntn, 4, 16, 4)          # [c][nt][kk][i16][e]
    back = planes.transpose(1, 3, 0, 2, 4).reshape(co, ci)              # [nt][i16] x [c][kk][e]
    assert np.array_equal(back, W)
    # what the kernel addresses (bytes): plane * (NTN * 1024) + (cb * 4 + wave) * 1024 + lane * 16, 16 bytes each, plane 0 .. nch -- plane
    # c + 1 is requested while chunk c runs, the last chunk included
    reach = max(plane * ntn * 1024 + tile * 1024 + lane * 16 + 16 for plane in (0, nch) for tile in (0, ntn - 1) for lane in (0, 63))
    assert reach == frag.size * 4
    assert not frag[nch * ntn * 256:].any(), "the look-ahead plane holds zeros"
    assert frag.size == (nch + 1) * ntn * 256


def test_pack_rejects_bad_arguments():
    lib = _lib.load()
    W = np.zeros((128, 64), np.float32)
    out = np.zeros(16, np.float32)
    fp = C.POINTER(C.c_float)
    wp, op = C.cast(W.ctypes.data_as(fp), C.c_void_p), C.cast(out.ctypes.data_as(fp), C.c_void_p)
    assert lib.cld_debug_pack_res_proj(wp, 128, 64, op, 16) < 0             # too small a buffer: nothing written
    assert not out.any()
    assert lib.cld_debug_pack_res_proj(wp, 120, 64, op, 1 << 20) < 0
    assert lib.cld_debug_pack_res_proj(wp, 128, 8, op, 1 << 20) < 0
