"""GPU tests (-m gpu) of index width, through the C ABI: the cases of tests/index_width_common.py -- every kernel family
where t * ld, c * stride and c * cap pass 2^31 bytes, 2^32 bytes and 2^32 elements, each held exactly to its reference,
a poisoned band next to every output region.  The model is tests/test_gpu_channel_major.py::test_offsets_are_64_bit: the
images (18.8 + 4.7 + 2 x 6.4 GB) are torch.empty allocations of which only the logical regions are ever written or read,
so a case costs milliseconds.  The entry points are called through dca.library() because the Context methods do not expose
the pitches (as tests/test_gpu_encoder_regimes.py::encode_at does).  tests/test_index_width_host.py runs the same cases on
the emulator, where a wrong offset is harmless: it passes before this file is run.

The chains (dega_hip_lzmh_encode_f32_dev, dega_hip_encode_levels_f32_dev, dega_hip_lzmh_decode_f32_dev) have only the
caller's arrays on the big pitch; their text_stride is an ordinary one, so the context's scratch stays small."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from __graft_entry__ import load_package

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_width_common as iw  # noqa: E402

pytestmark = pytest.mark.gpu

P, Z = C.c_void_p, C.c_size_t


class Device:
    """the backend of index_width_common over the library: torch tensors on the GPU, the device-resident entry points"""
    split_block_bytes = 1024  # the texts of 70 fields spread over two to four blocks; 2^20 blocks per channel

    def __init__(self, dca, ctx):
        import torch
        self.torch, self.dca, self.ctx, self.L = torch, dca, ctx, dca.library()
        self.images = {name: torch.empty(size, dtype=torch.uint8, device="cuda") for name, size in iw.IMAGES.items()}  # (never written as a whole)
        self.kept = []
        self.kinds = {"int32": torch.int32, "int64": torch.int64, "uint8": torch.uint8}

    def close(self):
        self.images.clear()
        self.torch.cuda.empty_cache()

    def call(self, fn, *args):
        ret = getattr(self.L, fn)(self.ctx._h, *args, self.ctx._stream())
        assert ret == 0, (fn, ret, self.ctx.last_error())

    # ---- memory ----
    def view(self, name, dtype, pitch):
        a = self.images[name].view(self.kinds[dtype]).view(-1, pitch)
        return iw.View(a, dtype, a.data_ptr())

    def put(self, a, r0, c0, block):
        assert block.dtype.itemsize == a.array.element_size()
        a.array[r0:r0 + block.shape[0], c0:c0 + block.shape[1]] = self.torch.from_numpy(np.array(block).view(a.dtype_name)).cuda()

    def get(self, a, r0, r1, c0, c1):
        self.torch.cuda.synchronize()
        return a.array[r0:r1, c0:c1].cpu().numpy()

    def dev(self, x):
        x = np.array(x)
        self.kept.append(self.torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda())  # (alive until forget(): the cases pass addresses on)
        return self.kept[-1]

    def forget(self):
        self.torch.cuda.synchronize()
        self.kept.clear()

    def host(self, d):
        self.torch.cuda.synchronize()
        return d.cpu().numpy()

    def ptr(self, d):
        return d.address if isinstance(d, iw.View) else d.data_ptr()

    @staticmethod
    def array(values, ctype):
        return (ctype * len(values))(*values)

    # ---- the entry points ----
    def aggregate(self, v, Cn, T, ld, N, a, ld_out, ranges=None):
        assert ranges is None  # (the ranges of output rows are the library's choice)
        self.call("dega_hip_aggregate_dev", v, Cn, T, ld, N, a, ld_out)

    def aggregate_levels(self, v, Cn, T, ld, levels, a, ld_out):
        self.call("dega_hip_aggregate_levels_dev", v, Cn, T, ld, self.array(levels, Z), len(levels), self.array(a, P), self.array(ld_out, Z))

    def aggregate_levels_var(self, v, Cn, T, ld, count, levels, a, ld_out, out_count, err):
        self.call("dega_hip_aggregate_levels_var_dev", v, Cn, T, ld, count, self.array(levels, Z), len(levels), self.array(a, P), self.array(ld_out, Z),
                  self.array(out_count, P), err)

    def encode(self, x, Cn, T, ld, ad, vs, out, cap, bits, err):
        self.call("dega_hip_encode_dev", x, Cn, T, ld, ad, vs, out, cap, bits, err)

    def encode64(self, x, Cn, T, ld, ad, vs, out, cap, bits, err):
        self.call("dega_hip_encode64_dev", x, Cn, T, ld, ad, vs, out, cap, bits, err)

    def encode_var(self, x, Cn, T, ld, count, ad, vs, out, cap, bits, err):
        self.call("dega_hip_encode_var_dev", x, Cn, T, ld, count, ad, vs, self.dca.SAMPLES_I32, out, cap, bits, err)

    def encode_segments(self, x, Cn, T, ld, ad, vs, cuts, out, cap, bits, err):
        state = self.torch.zeros(self.L.dega_hip_encode_state_bytes(Cn), dtype=self.torch.uint8, device="cuda")
        for k in range(len(cuts) - 1):
            flags = (1 if k > 0 else 0) | (2 if k + 2 < len(cuts) else 0)
            self.call("dega_hip_encode_segment_dev", x + 4 * cuts[k] * ld, Cn, cuts[k + 1] - cuts[k], ld, ad, vs, out, cap, bits, err, state.data_ptr(), flags)
        self.torch.cuda.synchronize()  # (state lives until the last launch has run)

    def decode(self, s, cap, bits, Cn, T, ld, ad, vs, x, err):
        self.call("dega_hip_decode_dev", s, cap, bits, Cn, T, ld, ad, vs, x, err)

    def decode_var(self, s, cap, bits, Cn, T, ld, ad, vs, x, counts, err):
        self.call("dega_hip_decode_var_dev", s, cap, bits, Cn, T, ld, ad, vs, x, counts, err)

    def decode64(self, s, cap, bits, Cn, T, ld, ad, vs, x, err):
        self.call("dega_hip_decode64_dev", s, cap, bits, Cn, T, ld, ad, vs, x, err)

    def encode_f32(self, v, Cn, T, ld, factor, ad, vs, out, cap, bits, err):
        self.call("dega_hip_encode_f32_dev", v, Cn, T, ld, factor, ad, vs, out, cap, bits, err)

    def encode_agg_f32(self, v, Cn, T, ld, N, factor, ad, vs, out, cap, bits, err):
        self.call("dega_hip_encode_agg_f32_dev", v, Cn, T, ld, N, factor, ad, vs, out, cap, bits, err)

    def decode_f32(self, s, cap, bits, Cn, T, ld, factor, ad, vs, v, counts, err):
        self.call("dega_hip_decode_f32_dev", s, cap, bits, Cn, T, ld, factor, ad, vs, v, counts or None, err)

    def normalize(self, v, Cn, T, ld, factor, vs, x, err):
        self.call("dega_hip_normalize_dev", v, Cn, T, ld, factor, vs, x, err)

    def denormalize(self, x, Cn, T, ld, factor, vs, v):
        self.call("dega_hip_denormalize_dev", x, Cn, T, ld, factor, vs, v)

    def with_store(self, form, fn, *args):
        """DEGA_CSV_STORE (read at every call) picks the form of the writer's stores"""
        before = os.environ.get("DEGA_CSV_STORE")
        os.environ["DEGA_CSV_STORE"] = "64" if form == "store64" else "8"
        try:
            self.call(fn, *args)
        finally:
            if before is None:
                del os.environ["DEGA_CSV_STORE"]
            else:
                os.environ["DEGA_CSV_STORE"] = before

    def csv_write(self, v, Cn, T, ld, d, column, sep, out, stride, lens, err, form):
        self.with_store(form, "dega_hip_csv_write_dev", v, Cn, T, ld, d, column, sep, out, stride, lens, err)

    def csv_write_var(self, v, Cn, T, ld, count, d, column, sep, out, stride, lens, err, form):
        self.with_store(form, "dega_hip_csv_write_var_dev", v, Cn, T, ld, count, d, column, sep, out, stride, lens, err)

    def csv_write_split(self, v, Cn, T, ld, count, d, column, sep, out, stride, lens, err, block_rows):
        self.call("dega_hip_csv_write_split_dev", v, Cn, T, ld, count or None, d, column, sep, out, stride, lens, err, block_rows)

    def csv_read(self, text, stride, lens, Cn, column, sep, v, max_T, ld, count, err):
        self.call("dega_hip_csv_read_dev", text, stride, lens, Cn, column, sep, v, max_T, ld, count, err)

    def csv_read_split(self, text, stride, lens, Cn, column, sep, v, max_T, ld, count, err, block_bytes):
        self.call("dega_hip_csv_read_split_dev", text, stride, lens, Cn, column, sep, v, max_T, ld, count, err, block_bytes)

    def lzmh_encode(self, text, stride, lens, Cn, out, cap, bits, err):
        self.call("dega_hip_lzmh_encode_dev", text, stride, lens, Cn, out, cap, bits, err)

    def lzmh_decode(self, s, cap, bits, Cn, out, stride, lens, err):
        self.call("dega_hip_lzmh_decode_dev", s, cap, bits, Cn, out, stride, lens, err)

    def lzmh_render(self, x, Cn, T, ld, out, stride, lens, err):
        self.call("dega_hip_lzmh_render_dev", x, Cn, T, ld, out, stride, lens, err)

    def compact(self, slabs, cap, offsets, Cn, packed, scatter):
        assert not scatter  # (the C ABI has the gather alone; the scatter runs inside the host jobs)
        self.call("dega_hip_compact_gather_dev", slabs, cap, offsets, Cn, packed)

    # ---- the chains ----
    def lzmh_encode_f32(self, v, Cn, T, ld, d, column, sep, text_stride, out, cap, bits, text_len, err):
        self.call("dega_hip_lzmh_encode_f32_dev", v, Cn, T, ld, d, column, sep, text_stride, out, cap, bits, text_len, err)

    def encode_levels_f32(self, v, Cn, T, ld, levels, factor, ad, vs, out, cap, bits, err):
        self.call("dega_hip_encode_levels_f32_dev", v, Cn, T, ld, self.array(levels, Z), len(levels), factor, ad, vs, self.array(out, P), self.array(cap, Z),
                  self.array(bits, P), self.array(err, P))

    def lzmh_decode_f32(self, s, cap, bits, Cn, text_stride, column, sep, v, max_T, ld, count, text_len, err):
        self.call("dega_hip_lzmh_decode_f32_dev", s, cap, bits, Cn, text_stride, column, sep, v, max_T, ld, count, text_len, err)


@pytest.fixture(scope="module")
def dca():
    return load_package()


@pytest.fixture(scope="module")
def B(dca):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    if torch.cuda.mem_get_info()[0] < iw.LIVE_BYTES + (1 << 30):
        pytest.skip("needs %.1f GB of free device memory for the sparse images" % (iw.LIVE_BYTES / 1e9))
    ctx = dca.Context(0)
    b = Device(dca, ctx)
    yield b
    torch.cuda.synchronize()
    b.close()
    del b
    ctx.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", iw.CASES + iw.GPU_ONLY, ids=lambda c: c[0])
def test_offsets_are_64_bit_on_the_device(B, case):
    iw.run(B, case)
