"""The fused DoubleConv blocks of the detection U-Net, one block at a time, against the oracle AND float64.

The three kernel families (kernels_det.hip: LDS-tiled; kernels_det_stream.hip: a wave per strip; kernels_det_rows.hip: a
workgroup per strip) are otherwise reached only through whole models of one form.  Here every block shape of the fused
table stands alone in a graph (tests/detblock_util.py) whose output is the block's own y / ypool / logit, with all sixteen
ReLU placements, decoder pad offsets 0 .. 22 of both parities, sizes on both sides of every tile, strip and segment
boundary, 1 .. 9 pages, NaN / Inf and signed zeros / subnormals.  Each case asserts, for every kernel family that has the
shape and for the per-operator kernels (det_fuse = 0):
  (a) the bits of the C oracle: uint32 views equal outside NaN positions, NaN positions identical;
  (b) the float64 bound of tests/f64_ref.py on every op of the graph (on the case's finite inputs), so that (a) bounds the
      kernels against float64 op by op;
  (c) which family ran: the per-launch kernel counters of an OcrEngine that runs the same block (same weights, flags, size,
      page count) closed to a detection-shaped graph — the expected class counted exactly one launch, the other two none.
      That includes the requests the row kernels decline (an odd pad offset; more than 8 pages under det_rows = 1).
The case list's own coverage is asserted without a GPU in tests/test_detection_blocks_cpu.py.

Run with:  python -m pytest -m gpu tests/test_gpu_detection_blocks.py
"""
import numpy as np
import pytest

import detblock_util as D
import f64_ref as R
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib
from oracle.nn import OracleGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _set(target, mode):
    for name, v in zip(("det_fuse", "det_stream", "det_rows"), mode):
        target.set_option(name, v)


@pytest.mark.parametrize("case", D.CASES, ids=[c.id for c in D.CASES])
def test_block_has_the_oracles_bits_in_every_kernel_family_that_takes_it(case):
    built = D.build(case)
    refs = {}
    for name, (buf, out) in built.graphs.items():
        _, slots = OracleGraph(buf).run_exact(built.x, return_slots=True)
        D.self_checks(case, built, slots)
        R.check_graph(buf, built.x_finite, case.id + " " + name)
        refs[name] = slots[out]
    models = {name: Model.load_bytes(buf) for name, (buf, _) in built.graphs.items()}
    eng = OcrEngine(detection_model=Model.load_bytes(built.companion))
    inps = [eng.prepare_input(ImageSource.from_tensor(np.ascontiguousarray(built.x_finite[i, 0, :, :, None]), DimOrder.Hwc))
            for i in range(case.n)]
    try:
        for mode in D.modes(case.shape):
            _set(_lib, mode)
            for name, m in models.items():
                got = np.ascontiguousarray(m.run(built.x).transpose(0, 2, 3, 1))      # NCHW from the executor
                D.same_bits(got, refs[name], "%s %s det_fuse / det_stream / det_rows %s" % (case.id, name, mode))
            # which family took the block
            _set(eng, mode)
            eng.enable_timing(2)
            eng.kernel_stats(reset=True)
            eng.detect_words_batch(inps)
            ks = eng.kernel_stats(reset=True)
            eng.enable_timing(0)
            want = D.expected_family(case, mode)
            seen = {f: ks[cls]["launches"] for f, cls in D.KERNEL_CLASS.items()}
            assert seen == {f: int(f == want) for f in D.KERNEL_CLASS}, (case.id, mode, want, seen)
    finally:
        _set(_lib, (1, 1, 1))
