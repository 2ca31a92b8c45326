"""haff_kv_prefix_broadcast (csrc/kv_broadcast.hip): positions 0 .. P-1 of a frame's K and V caches copied into the cache rows of the
prompts on that frame. Pure data movement, so every check is on bits: the destination equals src[frame_of][:, :P] and every other
byte of the destination allocation — positions >= P, and the guard rows around the K / V tensors — keeps its pattern."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

FRAME_OF = [2, 2, 0, 2, 0]          # B = 5 rows on F = 3 frames: frame 1 unused, the map not sorted
B, F = 5, 3
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _pattern(shape, dtype, dev, seed):
    """random bits (NaN payloads included: the kernel must not look at the values)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    it = torch.int16 if dtype != torch.float32 else torch.int32
    lim = 2 ** 15 if it == torch.int16 else 2 ** 31
    return torch.randint(-lim, lim - 1, shape, generator=g, dtype=it).view(dtype).to(dev)


@pytest.mark.parametrize("H", [64, 4096])
@pytest.mark.parametrize("P", [1, 7, 273])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_broadcast_equals_the_gather_and_writes_nothing_else(dev, dt, P, H):
    from haff import ops
    dtype = DTYPES[dt]
    tmax_src, tmax_dst = P, P + 5                      # the prefix fills the source cache exactly; the destination is longer
    ks = _pattern((F, tmax_src, H), dtype, dev, 1)
    vs = _pattern((F, tmax_src, H), dtype, dev, 2)
    # destination tensors cut out of larger allocations: one guard row in front and one behind
    kbuf = _pattern((B + 2, tmax_dst, H), dtype, dev, 3)
    vbuf = _pattern((B + 2, tmax_dst, H), dtype, dev, 4)
    k0, v0 = kbuf.clone(), vbuf.clone()
    kd, vd = kbuf[1:B + 1], vbuf[1:B + 1]
    fo = torch.tensor(FRAME_OF, dtype=torch.int32, device=dev)
    ops.kv_prefix_broadcast(ks, vs, kd, vd, fo, P)
    torch.cuda.synchronize()
    idx = torch.tensor(FRAME_OF, device=dev)
    for src, dst, buf, before in ((ks, kd, kbuf, k0), (vs, vd, vbuf, v0)):
        assert torch.equal(_bits(dst[:, :P]), _bits(src[idx][:, :P]))
        assert torch.equal(_bits(dst[:, P:]), _bits(before[1:B + 1, P:]))          # positions >= P
        assert torch.equal(_bits(buf[0]), _bits(before[0])) and torch.equal(_bits(buf[B + 1]), _bits(before[B + 1]))
    assert torch.equal(_bits(ks), _bits(_pattern((F, tmax_src, H), dtype, dev, 1)))   # the source is only read


def test_bad_arguments_are_refused_on_the_host(dev):
    import haff
    from haff import ops
    lib = haff.load_library()
    H, P, tmax = 64, 7, 12
    src = torch.zeros((2, F, tmax, H + 8), dtype=torch.bfloat16, device=dev)
    dst = torch.full((2, B, tmax, H + 8), 3.0, dtype=torch.bfloat16, device=dev)
    fo = torch.tensor(FRAME_OF, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def call(ks=src[0], vs=src[1], kd=dst[0], vd=dst[1], P=P, H=H, dtype=0, ss=None, ds=None, B_=B, F_=F):
        ss = src.stride(1) if ss is None else ss
        ds = dst.stride(1) if ds is None else ds
        return int(lib.haff_kv_prefix_broadcast(p(ks), p(vs), ss, p(kd), p(vd), ds, p(fo), B_, F_, P, H, dtype, st))
    # (the tensors are [.., H + 8] wide and the calls say H: the contract's H-stride between positions is what the ENTRY POINT assumes,
    # so these calls only probe its argument checks; tmax * (H + 8) >= P * H keeps every accepted call inside the allocations)
    assert call() == 0
    assert call(P=0) == -1 and call(P=-3) == -1
    # H * elem % 16 (the f32 calls give their row strides in f32 elements: half the bf16 tensors' rows, so they stay inside them)
    f32_rows = {"ss": src.stride(1) // 4, "ds": dst.stride(1) // 4, "dtype": 1}
    assert call(H=60) == -1 and call(H=4, **f32_rows) == 0 and call(H=3, **f32_rows) == -1 and call(H=4, dtype=3) == -1
    assert call(dtype=2) == -1 and call(dtype=7) == -1
    one = src.element_size()
    for name in ("ks", "vs", "kd", "vd"):                                              # a view offset by one element
        base = {"ks": src[0], "vs": src[1], "kd": dst[0], "vd": dst[1]}[name]
        assert call(**{name: base.reshape(-1)[1:]}) == -1, name
    assert one == 2
    assert call(ss=P * H - 8) == -1 and call(ds=P * H - 8) == -1 and call(ss=src.stride(1) + 1) == -1              # row strides
    assert call(B_=0) == -1 and call(F_=0) == -1
    assert int(lib.haff_kv_prefix_broadcast(None, p(src[1]), 1024, p(dst[0]), p(dst[1]), 1024, p(fo), B, F, P, H, 0, st)) == -1
    torch.cuda.synchronize()
    # the wrapper refuses a prefix longer than either cache before anything is launched
    ks = torch.zeros((F, 4, H), dtype=torch.bfloat16, device=dev)
    kd = torch.zeros((B, 9, H), dtype=torch.bfloat16, device=dev)
    with pytest.raises(AssertionError):
        ops.kv_prefix_broadcast(ks, ks.clone(), kd, kd.clone(), fo, 5)
    with pytest.raises(AssertionError):
        ops.kv_prefix_broadcast(ks, ks.clone(), kd, kd.clone(), fo.long(), 4)
