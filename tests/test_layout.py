"""The layout of the flat parameter vector, pinned without the library and without a device: the table in
mllp_amd/_lib.py (the Python twin of the one in csrc/internal.h, which pins itself by static_assert) against
GNNModel.state_dict(), against the literals that bench.py carries, and against the public header."""
import os
import re

from mllp_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_conv_slices_follow_state_dict():
    from mllp_amd.model import GNNModel
    walked, off = {}, 0                     # module name -> [start, stop) by key order and numel
    for key, t in GNNModel().state_dict().items():
        start, _ = walked.setdefault(key.split(".")[0], (off, off))
        off += t.numel()
        walked[key.split(".")[0]] = (start, off)
    assert list(walked) == list(_lib.CONV_NAMES) + ["fc"]
    for i, name in enumerate(_lib.CONV_NAMES):
        s = _lib.conv_param_slice(name)
        assert (s.start, s.stop, s.step) == (*walked[name], None), name
        assert _lib.conv_param_slice(i) == s
        assert s.stop - s.start == _lib.conv_param_count(_lib.CONV_CIN[i])
    assert walked["fc"] == (_lib.FC_OFFSET, _lib.NUM_PARAMS)
    lengths = [s.stop - s.start for s in map(_lib.conv_param_slice, _lib.CONV_NAMES)]
    assert sum(lengths) + walked["fc"][1] - walked["fc"][0] == _lib.NUM_PARAMS == off


def test_bench_literals_are_the_layout():
    """bench.py slices single convs out of the parameters with literals: `(dst_is_var, offset, ...)` tuples and a
    `[off:off + length]` slice in the loop over them."""
    with open(os.path.join(ROOT, "bench.py")) as fh:
        src = fh.read()
    found = set()
    for loop in re.finditer(r"for dst_is_var, (\w+)(?:, \w+)* in \(((?:\((?:False|True), \d+[^()]*\),? ?)+)\):", src):
        var, tuples = loop.group(1), loop.group(2)
        length = re.search(rf"\[{var}:{var} \+ (\d+)\]", src[loop.end():])
        assert length, f"no [{var}:{var} + N] slice after the loop over {var}"
        for off in re.findall(r"\((?:False|True), (\d+)", tuples):
            found.add((int(off), int(length.group(1))))
    want = {name: (s.start, s.stop - s.start) for name, s in ((n, _lib.conv_param_slice(n)) for n in _lib.CONV_NAMES[:4])}
    assert want == {"gconv2_s2w": (1392, 1104), "gconv2_w2s": (288, 1104), "gconv1_s2w": (144, 144), "gconv1_w2s": (0, 144)}
    assert found == set(want.values())


def test_header_num_params():
    with open(_lib.HEADER_PATH) as fh:
        m = re.search(r"^#define\s+MLLP_NUM_PARAMS\s+(\d+)", fh.read(), re.M)
    assert m and int(m.group(1)) == _lib.NUM_PARAMS
