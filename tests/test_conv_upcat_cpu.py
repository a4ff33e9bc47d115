"""gdkvm_conv_upcat_bias_act refuses bad arguments with the library's error codes before it touches the device or a pointer: the calls
below hand it addresses that are never dereferenced, on a machine that may have no GPU at all (a call that passed every check would end
at the library's device check, not in a launch)."""
import ctypes

ERR_SHAPE, ERR_DTYPE, ERR_ARG = -1, -2, -6                  # include/gdkvm.h
PACKED, BF16, F32 = 32, 1, 0


def test_argument_checks():
    from gdkvm_amd import build, ops
    build.build()
    lib = ops.load()
    assert (ops.CONV_PACKED_WEIGHTS, ops.BF16, ops.F32) == (PACKED, BF16, F32)
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15                  # a 16-byte aligned address

    def call(lo=p, x2=p, w=p, bias=p, res=None, y=p, n=1, c1=64, c2=64, h=14, w_=14, k=64, relu=1, kernel=PACKED, io=BF16):
        return lib.gdkvm_conv_upcat_bias_act(lo, x2, w, bias, res, y, n, c1, c2, h, w_, k, relu, kernel, io, None)

    assert call(io=F32) == ERR_DTYPE
    assert call(h=13) == ERR_SHAPE and b"even" in lib.gdkvm_last_error()
    assert call(w_=13) == ERR_SHAPE
    assert call(h=66, w_=66) == ERR_SHAPE                   # rows of more than 64 pixels
    assert call(c1=96) == ERR_SHAPE and call(c1=0) == ERR_SHAPE and call(c2=32) == ERR_SHAPE
    assert call(k=24) == ERR_SHAPE and call(n=-1) == ERR_SHAPE
    assert call(kernel=0) == ERR_ARG and call(kernel=5 | PACKED) == ERR_ARG      # the packed copy of the weights, wave grid by shape
    for name in ("lo", "x2", "w", "bias", "y"):
        assert call(**{name: None}) == ERR_ARG, name
        assert call(**{name: p + 8}) == ERR_ARG, name
    assert call(res=p + 2) == ERR_ARG
    assert call(n=0) == 0                                   # nothing to do: no device needed
    assert call(n=0, lo=None) == 0
