"""ocrs_amd — MI355X-native engine behind the robertknight/ocrs `OcrEngine` API.

Python mirror (ctypes) of the reference's public surface (ocrs/src/lib.rs:29-31,
111-301): `OcrEngine`, `OcrEngineParams`, `ImageSource`, `DimOrder`,
`DecodeMethod`, `TextLine`/`TextWord`/`TextChar`, plus `Model` for the
`trait Model` seam (ocrs/src/model.rs:6-17).  All compute happens in
libocrs_amd.so (HIP, gfx950); this module only marshals arrays.
"""
import collections
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import OcrsError, check, lib

__all__ = ["OcrEngine", "OcrEngineParams", "ImageSource", "ImageSourceError", "DimOrder", "DecodeMethod", "Model",
           "OcrInput", "TextLine", "TextWord", "TextChar", "OcrsError", "DEFAULT_ALPHABET", "EngineGroup", "line_frame",
           "Orientation", "orientation_vote", "unrotate_rects", "unrotate_lines", "work_size", "rescale_rects", "normalize_params", "rules_params", "speckle_params", "reverse_params", "binarize_params", "morph_params", "rank_params",
           "frame_params", "frame_choose", "uncrop_rects", "uncrop_boxes", "uncrop_lines",
           "measure_params", "measure_choose", "work_scale_for_text", "TextScale", "WORK_TEXT_HEIGHT_DEFAULT"]

# lib.rs:34 (with the EUR sign the comment at lib.rs:33 asks for)
DEFAULT_ALPHABET = " 0123456789!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~€ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"


class DimOrder:  # preprocess.rs:50-57
    Hwc = 0
    Chw = 1


class DecodeMethod:  # recognition.rs:198-205
    Greedy = ("greedy", 0)

    @staticmethod
    def BeamSearch(width):
        return ("beam", int(width))


class ImageSourceError(ValueError):  # preprocess.rs:38-46
    pass


class ImageSource:
    """preprocess.rs:61-124 — a borrowed view of u8 or f32 pixels, HWC or CHW."""

    def __init__(self, data, order):
        self.data = data
        self.order = order

    @staticmethod
    def from_bytes(buf, dimensions):
        width, height = dimensions
        ch = C.c_uint32(0)
        st = lib().ocrs_image_source_check_bytes(C.c_size_t(len(buf)), C.c_uint32(width), C.c_uint32(height), C.byref(ch))
        if st != 0:
            raise ImageSourceError(lib().ocrs_last_error().decode())
        arr = np.frombuffer(buf, dtype=np.uint8).reshape(height, width, ch.value)
        return ImageSource(arr, DimOrder.Hwc)

    @staticmethod
    def from_tensor(data, order):
        data = np.asarray(data)
        if data.ndim != 3:
            raise ImageSourceError("expected a 3-dimensional image tensor")
        chans = data.shape[2] if order == DimOrder.Hwc else data.shape[0]
        if chans not in (1, 3, 4):
            raise ImageSourceError("channel count is not 1, 3 or 4")
        if data.dtype not in (np.uint8, np.float32):
            raise ImageSourceError("pixels must be uint8 in [0,255] or float32 in [0,1]")
        return ImageSource(data, order)


class Model:
    """`trait Model` (model.rs:6-17): either an `.ocrsm` fixed graph executed by
    the HIP executor, or a Python callable (the reference's tests inject fake
    models through the same seam, lib.rs:339-422)."""

    def __init__(self, handle, keepalive=None):
        self._h = handle
        self._keep = keepalive

    @staticmethod
    def load_file(path):
        """`*.ocrsm` containers are read by the library; `*.onnx` files (the format the real
        ocrs models are published in, README.md:96-102) are lowered by `onnx_import` first."""
        if str(path).lower().endswith(".onnx"):
            from .onnx_import import import_onnx
            return Model.load_bytes(import_onnx(str(path)).to_bytes())
        h = C.c_void_p()
        check(lib().ocrs_model_load_file(str(path).encode(), C.byref(h)))
        return Model(h)

    @staticmethod
    def load_bytes(buf, device=None):
        """device=None: the process default (ocrs_set_device); an int places the weights on that HIP device."""
        h = C.c_void_p()
        if device is None:
            check(lib().ocrs_model_load_bytes(C.c_char_p(bytes(buf)), C.c_size_t(len(buf)), C.byref(h)))
        else:
            check(lib().ocrs_model_load_bytes_on_device(C.c_char_p(bytes(buf)), C.c_size_t(len(buf)), C.c_int(int(device)),
                                                        C.byref(h)))
        return Model(h)

    def device(self):
        d = C.c_int(-1)
        check(lib().ocrs_model_device(self._h, C.byref(d)))
        return d.value

    @staticmethod
    def from_callable(input_shape, fn):
        """input_shape: NCHW with None for symbolic dims; fn(np [N,C,H,W] f32) -> np (<= 4 dims)."""
        libc = C.CDLL(None)
        libc.malloc.restype = C.c_void_p
        libc.malloc.argtypes = [C.c_size_t]
        err = []

        def _run(user, inp, in_shape, out, out_shape, out_ndim):
            try:
                shp = [in_shape[i] for i in range(4)]
                x = np.ctypeslib.as_array(inp, shape=(int(np.prod(shp)),)).reshape(shp).copy()
                y = np.ascontiguousarray(fn(x), dtype=np.float32)
                if y.ndim < 1 or y.ndim > 4:
                    return 2
                p = libc.malloc(max(y.nbytes, 4))
                C.memmove(p, y.ctypes.data, y.nbytes)
                out[0] = C.cast(p, C.POINTER(C.c_float))
                for i, d in enumerate(y.shape):
                    out_shape[i] = d
                out_ndim[0] = y.ndim
                return 0
            except Exception as e:  # surfaces as ModelRunError::RunFailed
                err.append(e)
                return 1

        cb = _lib.RUN_FN(_run)
        shape = (C.c_int64 * 4)(*[-1 if d is None else int(d) for d in input_shape])
        h = C.c_void_p()
        check(lib().ocrs_model_from_callback(shape, cb, None, C.byref(h)))
        return Model(h, keepalive=(cb, err))

    def input_shape(self):
        dims = (C.c_int64 * 4)()
        fixed = (C.c_uint8 * 4)()
        check(lib().ocrs_model_input_shape(self._h, dims, fixed))
        return [int(dims[i]) if fixed[i] else None for i in range(4)]

    def run(self, nchw, timing=False):
        x = np.ascontiguousarray(nchw, dtype=np.float32)
        assert x.ndim == 4
        shape = (C.c_int64 * 4)(*x.shape)
        out = C.POINTER(C.c_float)()
        oshape = (C.c_int64 * 4)()
        ond = C.c_int(0)
        opts = _lib.RunOptions(1 if timing else 0)
        check(lib().ocrs_model_run(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), shape, C.byref(opts), C.byref(out),
                                   oshape, C.byref(ond)))
        shp = [int(oshape[i]) for i in range(ond.value)]
        y = np.ctypeslib.as_array(out, shape=(int(np.prod(shp)),)).reshape(shp).copy()
        lib().ocrs_buffer_free(out)
        return y

    def flops(self, n, h, w):
        shape = (C.c_int64 * 4)(n, 1, h, w)
        f = C.c_double(0)
        check(lib().ocrs_model_flops(self._h, shape, C.byref(f)))
        return f.value

    def __del__(self):
        try:
            if self._h:
                lib().ocrs_model_free(self._h)
                self._h = None
        except Exception:
            pass


NUMERICS = {"exact": 0, "relaxed": 1, "reduced": 2}   # ocrs_numerics


class OcrEngineParams:  # lib.rs:38-71
    def __init__(self, detection_model=None, recognition_model=None, debug=False, decode_method=DecodeMethod.Greedy,
                 alphabet=None, allowed_chars=None, numerics="exact", coalesce=0, coalesce_pages=0, coalesce_window_us=0,
                 layout_threads=0, rec_max_pixels=0, options=None):
        # numerics / coalesce*: ocrs_engine_params fields without a reference counterpart (0 = default); while an engine with
        # numerics != "exact" is alive, every call on its device runs its kernels one at a time (include/ocrs_amd.h);
        # options: {name: value} applied to the new engine with ocrs_engine_set_option
        self.numerics = numerics
        self.coalesce = coalesce
        self.coalesce_pages = coalesce_pages
        self.coalesce_window_us = coalesce_window_us
        self.layout_threads = layout_threads
        self.rec_max_pixels = rec_max_pixels
        self.options = dict(options or {})
        self.detection_model = detection_model
        self.recognition_model = recognition_model
        self.debug = debug
        self.decode_method = decode_method
        self.alphabet = alphabet
        self.allowed_chars = allowed_chars


class OcrInput:
    """lib.rs:125-128 — the prepared grey page, resident in HBM."""

    def __init__(self, handle):
        self._h = handle

    @property
    def shape(self):
        h, w = C.c_int(0), C.c_int(0)
        check(lib().ocrs_page_dims(self._h, C.byref(h), C.byref(w)))
        return (1, h.value, w.value)

    def image(self):
        _, h, w = self.shape
        out = np.empty((1, h, w), np.float32)
        check(lib().ocrs_page_image(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def __del__(self):
        try:
            if self._h:
                lib().ocrs_page_free(self._h)
                self._h = None
        except Exception:
            pass


class TextChar:  # text_items.rs:48-54
    __slots__ = ("char", "rect", "logp")

    def __init__(self, char, rect, logp=None):
        self.char = char
        self.rect = rect  # (top, left, bottom, right)
        self.logp = logp  # log-prob of the CTC step the char came from (float32), None when unscored

    @property
    def confidence(self):
        """exp(logp), or None when unscored."""
        return None if self.logp is None else math.exp(float(self.logp))


class _TextItem:
    def __init__(self, chars):
        self._chars = chars

    def chars(self):
        return self._chars

    @property
    def confidence(self):
        """exp of the mean of the chars' logp, in float64 (a line's mean includes its spaces); None when unscored."""
        if not self._chars or any(c.logp is None for c in self._chars):
            return None
        return math.exp(math.fsum(float(c.logp) for c in self._chars) / len(self._chars))

    def bounding_rect(self):
        a = np.array([c.rect for c in self._chars])
        return (int(a[:, 0].min()), int(a[:, 1].min()), int(a[:, 2].max()), int(a[:, 3].max()))

    def rotated_rect(self):
        """text_items.rs:18-30 -> (center.x, center.y, up.x, up.y, width, height)."""
        a = np.ascontiguousarray(np.array([c.rect for c in self._chars], np.int32).reshape(-1, 4))
        out = (C.c_float * 6)()
        check(lib().ocrs_text_item_rotated_rect(a.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(len(a)), out))
        return np.array(list(out), np.float32)

    def __str__(self):
        return "".join(c.char for c in self._chars)


def rotated_rect_corners(rect6):
    """RotatedRect::corners -> [[x, y] x 4] floats."""
    r = (C.c_float * 6)(*[float(v) for v in rect6])
    out = (C.c_float * 8)()
    check(lib().ocrs_rotated_rect_corners(r, out))
    return [[out[2 * i], out[2 * i + 1]] for i in range(4)]


class TextWord(_TextItem):  # text_items.rs:92-107
    pass


class TextLine(_TextItem):  # text_items.rs:61-82
    def __init__(self, chars, score=None):
        assert chars, "Text lines must not be empty"
        super().__init__(chars)
        self.score = score  # float64 line score (include/ocrs_amd.h), None when unscored

    def words(self):
        out, cur = [], []
        for c in self._chars:
            if c.char == " ":
                if cur:
                    out.append(TextWord(cur))
                cur = []
            else:
                cur.append(c)
        if cur:
            out.append(TextWord(cur))
        return out


def _rects_to_array(rects):
    a = np.ascontiguousarray(np.asarray(rects, dtype=np.float32).reshape(-1, 6))
    return a


def _take(ptr, n, dtype):
    """Copies n items out of a malloc'ed result array and frees it."""
    out = np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].astype(dtype, copy=True)
    lib().ocrs_buffer_free(ptr)
    return out


def _take_rects(ptr, n):
    """_take for n word rects -> float32 [n, 6]."""
    return _take(ptr, n * 6, np.float32).reshape(-1, 6)


def _page_array(inputs):
    """The pages of OcrInputs as the `const ocrs_page* const*` argument of a batch call."""
    return (C.c_void_p * len(inputs))(*[i._h for i in inputs])


def _new_inputs(out, n):
    """The n pages a batch call wrote into its `ocrs_page**` argument, each owned by a new OcrInput."""
    return [OcrInput(C.c_void_p(out[i])) for i in range(n)]


def _tile_overlap(tiled):
    """The `tiled` keyword of the detection calls -> None (untiled) or the overlap argument of the _tiled entry points:
    False / None: untiled; True: the default overlap (-1); an int: that many pixels (0 is a valid overlap)."""
    if tiled is False or tiled is None:
        return None
    if tiled is True:
        return -1
    v = int(tiled)
    if v < 0:
        raise ValueError("tiled: an overlap in pixels, or True for the default")
    return v


def tile_plan(page_hw, model_hw, overlap=None):
    """ocrs_detection_tile_plan (host only): the tiles a page of page_hw is cut into for a detection model whose input is
    model_hw -> (origin_y [ny], bound_y [ny + 1], origin_x [nx], bound_x [nx + 1]), int32.  Tile (i, j)
    starts at (origin_y[i], origin_x[j]) and owns rows bound_y[i] .. bound_y[i + 1], columns bound_x[j] .. bound_x[j + 1].
    overlap=None: the default (_lib.TILE_OVERLAP_DEFAULT)."""
    ny, nx = C.c_size_t(0), C.c_size_t(0)
    p = [C.POINTER(C.c_int32)() for _ in range(4)]
    check(lib().ocrs_detection_tile_plan(int(page_hw[0]), int(page_hw[1]), int(model_hw[0]), int(model_hw[1]),
                                         -1 if overlap is None else int(overlap), C.byref(ny), C.byref(nx), *[C.byref(x) for x in p]))
    return tuple(_take(x, k, np.int32) for x, k in zip(p, (ny.value, ny.value + 1, nx.value, nx.value + 1)))


class LineFrame:
    """ocrs_line_frame's outputs: empty, axis float64 [2], extents float64 [4] (s_min, s_max, t_min,
    t_max), rw, coef float32 [6] (x0, ax, bx, y0, ay, by), ranges int32 [n, 4] (c0, c1, r0, r1 per word)."""
    __slots__ = ("empty", "axis", "extents", "rw", "coef", "ranges")


def line_frame(words, rec_height=64):
    """ocrs_line_frame (host only): the frame a rectified crop gives one line of word rects for a recogniser of input
    height rec_height."""
    a = _rects_to_array(words)
    axis, ext, coef = np.zeros(2, np.float64), np.zeros(4, np.float64), np.zeros(6, np.float32)
    ranges = np.zeros((len(a), 4), np.int32)
    rw, empty = C.c_uint32(0), C.c_int(0)
    check(lib().ocrs_line_frame(a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(len(a)), C.c_int(int(rec_height)),
                                axis.ctypes.data_as(C.POINTER(C.c_double)), ext.ctypes.data_as(C.POINTER(C.c_double)), C.byref(rw),
                                coef.ctypes.data_as(C.POINTER(C.c_float)), ranges.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(empty)))
    f = LineFrame()
    f.empty, f.axis, f.extents, f.rw, f.coef, f.ranges = bool(empty.value), axis, ext, int(rw.value), coef, ranges
    return f


def line_char_boxes(words, ctc_input_len, positions, rec_height=64):
    """ocrs_line_char_boxes (host only): the page boxes of a rectified line's chars from its CTC steps' positions ->
    (rects int32 [n, 4] (top, left, bottom, right), kept bool [n])."""
    a = _rects_to_array(words)
    pos = np.ascontiguousarray(positions, np.uint32)
    rects, kept = np.zeros((len(pos), 4), np.int32), np.zeros(len(pos), np.uint8)
    check(lib().ocrs_line_char_boxes(a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(len(a)), C.c_int(int(rec_height)),
                                     C.c_uint32(int(ctc_input_len)), pos.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(len(pos)),
                                     rects.ctypes.data_as(C.POINTER(C.c_int32)), kept.ctypes.data_as(C.POINTER(C.c_uint8))))
    return rects, kept.astype(bool)


class Orientation:
    """ocrs_engine_detect_orientation's outputs: quarter_turns (the counter-clockwise quarter turns that
    make the page read), vote float64 [2] (horizontal, vertical), scores float64 [4] (mean char log-prob per turn; NaN for
    the two turns that were not candidates, -inf for a candidate without chars), n_chars uint32 [4]."""
    __slots__ = ("quarter_turns", "vote", "scores", "n_chars")

    def __repr__(self):
        return "Orientation(quarter_turns=%d, vote=%s, scores=%s, n_chars=%s)" % (
            self.quarter_turns, self.vote.tolist(), self.scores.tolist(), self.n_chars.tolist())


def orientation_vote(rects):
    """ocrs_orientation_vote (host only): the word-shape vote over word rects -> float64 [2]: the summed widths of the
    words wider than tall, the summed heights of the others.  The page reads horizontally iff vote[0] >= vote[1]."""
    a = _rects_to_array(rects)
    out = np.zeros(2, np.float64)
    check(lib().ocrs_orientation_vote(a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(len(a)),
                                      out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def unrotate_rects(rects, page_hw, k):
    """ocrs_unrotate_rects (host only): word rects found on np.rot90(page, k) -> the same rects in the frame of the
    page_hw = (height, width) page itself, float32 [n, 6] (a copy)."""
    a = _rects_to_array(rects).copy()
    check(lib().ocrs_unrotate_rects(a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(len(a)), C.c_int(int(page_hw[0])),
                                    C.c_int(int(page_hw[1])), C.c_int(int(k))))
    return a


def unrotate_boxes(boxes, page_hw, k):
    """ocrs_unrotate_chars on bare boxes: int32 [n, 4] (top, left, bottom, right) on np.rot90(page, k) -> in the page's frame."""
    b = np.asarray(boxes, np.int32).reshape(-1, 4)
    arr = (_lib.TextCharC * max(len(b), 1))()
    for i, (t, l, bo, r) in enumerate(b.tolist()):
        arr[i] = _lib.TextCharC(0, t, l, bo, r)
    check(lib().ocrs_unrotate_chars(arr, C.c_size_t(len(b)), C.c_int(int(page_hw[0])), C.c_int(int(page_hw[1])), C.c_int(int(k))))
    return np.array([[arr[i].top, arr[i].left, arr[i].bottom, arr[i].right] for i in range(len(b))], np.int32).reshape(-1, 4)


def unrotate_lines(text_lines, page_hw, k):
    """recognize_text's output on np.rot90(page, k) -> new TextLines (None stays None) whose char boxes are in the frame of
    the page_hw = (height, width) page itself (ocrs_unrotate_chars); text, log-probs and scores are kept."""
    out = []
    for t in text_lines:
        if t is None:
            out.append(None)
            continue
        boxes = unrotate_boxes([c.rect for c in t.chars()], page_hw, k)
        out.append(TextLine([TextChar(c.char, tuple(int(v) for v in b), c.logp) for c, b in zip(t.chars(), boxes)], t.score))
    return out


def work_size(page_hw, scale=None, max_side=None):
    """ocrs_work_size (host only): the work size (height, width) of a page_hw = (height, width) page.
    scale: each side is floor(side * scale + 0.5), kept within 1 .. 65535.  max_side=N: scale = min(1, N / max(H, W)): the
    longest side becomes N at most and a smaller page keeps its size.  Exactly one of the two."""
    if (scale is None) == (max_side is None):
        raise ValueError("work_size: give scale or max_side")
    h, w = int(page_hw[0]), int(page_hw[1])
    if max_side is not None:
        scale = min(1.0, float(max_side) / float(max(h, w)))
    oh, ow = C.c_int(0), C.c_int(0)
    check(lib().ocrs_work_size(C.c_int(h), C.c_int(w), C.c_double(float(scale)), C.byref(oh), C.byref(ow)))
    return oh.value, ow.value


def rescale_rects(rects, from_hw, to_hw):
    """ocrs_rescale_rects (host only): word rects of the from_hw = (height, width) frame of a picture -> the same rects in
    its to_hw frame, float32 [n, 6] (a copy).  Equal sizes keep every bit."""
    a = _rects_to_array(rects).copy()
    check(lib().ocrs_rescale_rects(a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(len(a)), C.c_int(int(from_hw[0])),
                                   C.c_int(int(from_hw[1])), C.c_int(int(to_hw[0])), C.c_int(int(to_hw[1]))))
    return a


def normalize_params(tile=None, polarity=None, flatten=None, levels=None):
    """ocrs_normalize_params as a dict: ocrs_normalize_params_default (tile 64, polarity "auto", flatten and
    levels on) with the given fields replaced, checked by ocrs_normalize_params_check (host only)."""
    p = _normalize_struct(tile, polarity, flatten, levels)
    check(lib().ocrs_normalize_params_check(C.byref(p)))
    return {"tile": int(p.tile), "polarity": [k for k, v in _lib.POLARITIES.items() if v == p.polarity][0],
            "flatten": bool(p.flatten), "levels": bool(p.levels)}


def _normalize_struct(tile=None, polarity=None, flatten=None, levels=None):
    p = _lib.NormalizeParams()
    check(lib().ocrs_normalize_params_default(C.byref(p)))
    if tile is not None:
        p.tile = int(tile)
    if polarity is not None:
        if polarity not in _lib.POLARITIES:
            raise ValueError("normalize: polarity is one of %s" % ", ".join(_lib.POLARITIES))
        p.polarity = _lib.POLARITIES[polarity]
    if flatten is not None:
        p.flatten = 1 if flatten else 0
    if levels is not None:
        p.levels = 1 if levels else 0
    return p


def rules_params(min_length=None, max_thickness=None, margin=None, threshold=None, paper=None):
    """ocrs_rules_params as a dict: ocrs_rules_params_default (min_length 96, max_thickness 8, margin 1,
    threshold 0, paper None = measured) with the given fields replaced, checked by ocrs_rules_params_check (host only)."""
    p = _rules_struct(min_length, max_thickness, margin, threshold, paper)
    check(lib().ocrs_rules_params_check(C.byref(p)))
    return {"min_length": int(p.min_length), "max_thickness": int(p.max_thickness), "margin": int(p.margin), "threshold": float(p.threshold),
            "paper": None if p.paper != p.paper else float(p.paper)}


def _rules_struct(min_length=None, max_thickness=None, margin=None, threshold=None, paper=None):
    p = _lib.RulesParams()
    check(lib().ocrs_rules_params_default(C.byref(p)))
    if min_length is not None:
        p.min_length = int(min_length)
    if max_thickness is not None:
        p.max_thickness = int(max_thickness)
    if margin is not None:
        p.margin = int(margin)
    if threshold is not None:
        p.threshold = float(threshold)
    if paper is not None:
        p.paper = float(paper)
    return p


def speckle_params(max_area=None, max_hole=None, keep_near=None, threshold=None, paper=None, ink_level=None):
    """ocrs_speckle_params as a dict: ocrs_speckle_params_default (max_area 4, max_hole 0, keep_near 0,
    threshold 0, paper and ink_level None = measured) with the given fields replaced, checked by ocrs_speckle_params_check
    (host only)."""
    p = _speckle_struct(max_area, max_hole, keep_near, threshold, paper, ink_level)
    check(lib().ocrs_speckle_params_check(C.byref(p)))
    return {"max_area": int(p.max_area), "max_hole": int(p.max_hole), "keep_near": int(p.keep_near), "threshold": float(p.threshold),
            "paper": None if p.paper != p.paper else float(p.paper), "ink_level": None if p.ink_level != p.ink_level else float(p.ink_level)}


def _speckle_struct(max_area=None, max_hole=None, keep_near=None, threshold=None, paper=None, ink_level=None):
    p = _lib.SpeckleParams()
    check(lib().ocrs_speckle_params_default(C.byref(p)))
    if max_area is not None:
        p.max_area = int(max_area)
    if max_hole is not None:
        p.max_hole = int(max_hole)
    if keep_near is not None:
        p.keep_near = int(keep_near)
    if threshold is not None:
        p.threshold = float(threshold)
    if paper is not None:
        p.paper = float(paper)
    if ink_level is not None:
        p.ink_level = float(ink_level)
    return p


def binarize_params(radius=None, k=None, keep_ink=None, ink_level=None, paper=None):
    """ocrs_binarize_params as a dict: ocrs_binarize_params_default (radius 15, k_q8 87, keep_ink False,
    ink_level and paper None = -0.5 and +0.5) with the given fields replaced (k rounded to 1/256: k_q8), checked by
    ocrs_binarize_params_check (host only)."""
    p = _binarize_struct(radius, k, keep_ink, ink_level, paper)
    check(lib().ocrs_binarize_params_check(C.byref(p)))
    return {"radius": int(p.radius), "k_q8": int(p.k_q8), "keep_ink": bool(p.keep_ink),
            "ink_level": None if p.ink_level != p.ink_level else float(p.ink_level), "paper": None if p.paper != p.paper else float(p.paper)}


def _binarize_struct(radius=None, k=None, keep_ink=None, ink_level=None, paper=None):
    p = _lib.BinarizeParams()
    check(lib().ocrs_binarize_params_default(C.byref(p)))
    if radius is not None:
        p.radius = int(radius)
    if k is not None:
        q = math.floor(float(k) * 256.0 + 0.5)   # Sauvola's k in 1/256; out of range is the library's to refuse
        p.k_q8 = int(max(-1, min(q, 257)))
    if keep_ink is not None:
        p.keep_ink = 1 if keep_ink else 0
    if ink_level is not None:
        p.ink_level = float(ink_level)
    if paper is not None:
        p.paper = float(paper)
    return p


MORPH_OPS = ("thicken", "thin", "close", "open")   # include/ocrs_amd.h OCRS_MORPH_*


def morph_params(op=None, rx=None, ry=None):
    """ocrs_morph_params as a dict: ocrs_morph_params_default (close, rx 1, ry 1) with the given fields
    replaced (op by name; ry=None with an rx given means ry = rx), checked by ocrs_morph_params_check (host only)."""
    p = _morph_struct(op, rx, ry)
    check(lib().ocrs_morph_params_check(C.byref(p)))
    return {"op": MORPH_OPS[p.op], "rx": int(p.rx), "ry": int(p.ry)}


def _morph_struct(op=None, rx=None, ry=None):
    p = _lib.MorphParams()
    check(lib().ocrs_morph_params_default(C.byref(p)))
    if op is not None:
        if op not in MORPH_OPS:
            raise ValueError("morph: op is one of %s, not %r" % (", ".join(MORPH_OPS), op))
        p.op = MORPH_OPS.index(op)
    if rx is not None:
        p.rx = int(rx)   # out of range is the library's to refuse
        if ry is None:
            p.ry = int(rx)
    if ry is not None:
        p.ry = int(ry)
    return p


def rank_params(rx=None, ry=None, percent=None, tail=None):
    """ocrs_rank_params as a dict: ocrs_rank_params_default (rx 1, ry 1, percent 50, tail 20) with the
    given fields replaced (ry=None with an rx given means ry = rx), checked by ocrs_rank_params_check (host only)."""
    p = _rank_struct(rx, ry, percent, tail)
    check(lib().ocrs_rank_params_check(C.byref(p)))
    return {"rx": int(p.rx), "ry": int(p.ry), "percent": int(p.percent), "tail": int(p.tail)}


def _rank_struct(rx=None, ry=None, percent=None, tail=None):
    p = _lib.RankParams()
    check(lib().ocrs_rank_params_default(C.byref(p)))
    if rx is not None:
        p.rx = int(rx)   # out of range is the library's to refuse
        if ry is None:
            p.ry = int(rx)
    if ry is not None:
        p.ry = int(ry)
    if percent is not None:
        p.percent = int(percent)
    if tail is not None:
        p.tail = int(tail)
    return p


FRAME_SIDES = {"L": 1, "T": 2, "R": 4, "B": 8}   # include/ocrs_amd.h ocrs_frame_params.sides


def _frame_sides(sides):
    """sides as the bits of ocrs_frame_params, from an int or from letters out of "LTRB" (any case)."""
    if isinstance(sides, str):
        if not sides or any(c not in FRAME_SIDES for c in sides.upper()):
            raise ValueError("clean_frame: sides are letters out of LTRB, not %r" % (sides,))
        bits = 0
        for c in sides.upper():
            bits |= FRAME_SIDES[c]
        return bits
    return int(sides)


def frame_params(depth=None, sides=None, min_area=None, threshold=None, paper=None):
    """ocrs_frame_params as a dict: ocrs_frame_params_default (depth 128, sides 15, min_area 0, threshold 0,
    paper None = measured) with the given fields replaced (sides: the bits, or letters out of "LTRB"), checked by
    ocrs_frame_params_check (host only)."""
    p = _frame_struct(depth, sides, min_area, threshold, paper)
    check(lib().ocrs_frame_params_check(C.byref(p)))
    return {"depth": int(p.depth), "sides": int(p.sides), "min_area": int(p.min_area), "threshold": float(p.threshold),
            "paper": None if p.paper != p.paper else float(p.paper)}


def _frame_struct(depth=None, sides=None, min_area=None, threshold=None, paper=None):
    p = _lib.FrameParams()
    check(lib().ocrs_frame_params_default(C.byref(p)))
    if depth is not None:
        p.depth = int(depth)   # out of range is the library's to refuse
    if sides is not None:
        p.sides = _frame_sides(sides)
    if min_area is not None:
        p.min_area = int(min_area)
    if threshold is not None:
        p.threshold = float(threshold)
    if paper is not None:
        p.paper = float(paper)
    return p


def _choice_struct(min_count=None, pad=None, gutter_min_width=None, gutter_max_ink=None):
    p = _lib.FrameChoiceParams()
    check(lib().ocrs_frame_choice_params_default(C.byref(p)))
    for name, v in (("min_count", min_count), ("pad", pad), ("gutter_min_width", gutter_min_width), ("gutter_max_ink", gutter_max_ink)):
        if v is not None:
            setattr(p, name, int(v))
    return p


def frame_choose(page_hw, col_ink, row_ink, min_count=None, pad=None, gutter_min_width=None, gutter_max_ink=None):
    """ocrs_frame_choose (host only): the content box and the gutter of a page_hw = (height, width) page
    from its ink profiles (uint32 [width], uint32 [height]: OcrEngine.ink_profiles) -> {"found", "x0", "y0", "x1", "y1",
    "gutter_x"}.  The box is half open and is the whole page when nothing was found; gutter_x is the first column of the
    right page of a spread, -1 without one.  Defaults: min_count 1, pad 16, gutter_min_width 8, gutter_max_ink 0."""
    h, w = int(page_hw[0]), int(page_hw[1])
    cols, rows = np.ascontiguousarray(col_ink, np.uint32), np.ascontiguousarray(row_ink, np.uint32)
    if cols.shape != (w,) or rows.shape != (h,):
        raise ValueError("frame_choose: the profiles of a %d x %d page are [%d] and [%d]" % (h, w, w, h))
    p = _choice_struct(min_count, pad, gutter_min_width, gutter_max_ink)
    out = _lib.FrameChoice()
    check(lib().ocrs_frame_choose(C.c_int(h), C.c_int(w), cols.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  rows.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(p), C.byref(out)))
    return out.as_dict()


def measure_params(threshold=None, min_area=None):
    """ocrs_measure_params as a dict: ocrs_measure_params_default (threshold 0, min_area 4) with the given
    fields replaced, checked by ocrs_measure_params_check (host only)."""
    p = _measure_struct(threshold, min_area)
    check(lib().ocrs_measure_params_check(C.byref(p)))
    return {"threshold": float(p.threshold), "min_area": int(p.min_area)}


def _measure_struct(threshold=None, min_area=None):
    p = _lib.MeasureParams()
    check(lib().ocrs_measure_params_default(C.byref(p)))
    if threshold is not None:
        p.threshold = float(threshold)
    if min_area is not None:
        p.min_area = int(max(-1, min(int(min_area), 1 << 30)))   # out of range is the library's to refuse
    return p


def reverse_params(min_height=None, min_width=None, min_fill=None, min_holes=None, max_hole=None, threshold=None):
    """ocrs_reverse_params as a dict: ocrs_reverse_params_default (min_height 32, min_width 64, min_fill
    0.4, min_holes 3, max_hole 0 = no limit, threshold 0; the five are uncalibrated) with the given fields replaced, checked
    by ocrs_reverse_params_check (host only)."""
    p = _reverse_struct(min_height, min_width, min_fill, min_holes, max_hole, threshold)
    check(lib().ocrs_reverse_params_check(C.byref(p)))
    return {"min_height": int(p.min_height), "min_width": int(p.min_width), "min_fill": float(p.min_fill), "min_holes": int(p.min_holes),
            "max_hole": int(p.max_hole), "threshold": float(p.threshold)}


def _reverse_struct(min_height=None, min_width=None, min_fill=None, min_holes=None, max_hole=None, threshold=None):
    p = _lib.ReverseParams()
    check(lib().ocrs_reverse_params_default(C.byref(p)))
    clip = lambda v: int(max(-1, min(int(v), (1 << 31) - 1)))   # out of range is the library's to refuse
    if min_height is not None:
        p.min_height = clip(min_height)
    if min_width is not None:
        p.min_width = clip(min_width)
    if min_fill is not None:
        p.min_fill = float(min_fill)
    if min_holes is not None:
        p.min_holes = clip(min_holes)
    if max_hole is not None:
        p.max_hole = clip(max_hole)
    if threshold is not None:
        p.threshold = float(threshold)
    return p


TextScale = collections.namedtuple("TextScale", ("stroke", "text_height", "support", "blank"))
TextScale.__doc__ = """ocrs_text_scale (DESIGN.md §7.14): stroke and text_height in pixels (0: none found), support (the
components that entered the median) and blank (bool: support == 0)."""
WORK_TEXT_HEIGHT_DEFAULT = _lib.WORK_TEXT_HEIGHT_DEFAULT   # include/ocrs_amd.h OCRS_WORK_TEXT_HEIGHT_DEFAULT
WORK_TEXT_SCALE_RANGE = (0.125, 4.0)   # what detect_words(work_text_height=...) keeps the derived scale within


def measure_choose(info, min_height_strokes=None):
    """ocrs_measure_choose (host only): the scale of a page from its measurement (OcrEngine.measure's dict)
    -> TextScale.  min_height_strokes: None is the default, 0.5."""
    p = _lib.MeasureChoiceParams()
    check(lib().ocrs_measure_choice_params_default(C.byref(p)))
    if min_height_strokes is not None:
        p.min_height_strokes = float(min_height_strokes)
    rec = _lib.MeasureInfo.from_dict(info)
    out = _lib.TextScaleC()
    check(lib().ocrs_measure_choose(C.byref(rec), C.byref(p), C.byref(out)))
    return TextScale(int(out.stroke), int(out.text_height), int(out.support), bool(out.blank))


def work_scale_for_text(text_height, target_height=None, min_scale=WORK_TEXT_SCALE_RANGE[0], max_scale=WORK_TEXT_SCALE_RANGE[1]):
    """ocrs_work_scale_for_text (host only): the scale that brings text of text_height pixels to target_height (None:
    WORK_TEXT_HEIGHT_DEFAULT), kept within [min_scale, max_scale]; 1.0 for a blank page (text_height 0).  Feeds work_size."""
    out = C.c_double(0.0)
    target = WORK_TEXT_HEIGHT_DEFAULT if target_height is None else target_height
    check(lib().ocrs_work_scale_for_text(C.c_int(int(text_height)), C.c_double(float(target)), C.c_double(float(min_scale)),
                                         C.c_double(float(max_scale)), C.byref(out)))
    return out.value


def uncrop_rects(rects, origin):
    """ocrs_uncrop_rects (host only): word rects found on a page cut out at origin = (x0, y0) -> the same rects in the frame
    of the page it was cut from, float32 [n, 6] (a copy)."""
    a = _rects_to_array(rects).copy()
    check(lib().ocrs_uncrop_rects(a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(len(a)), C.c_int(int(origin[0])), C.c_int(int(origin[1]))))
    return a


def uncrop_boxes(boxes, origin):
    """ocrs_uncrop_chars on bare boxes: int32 [n, 4] (top, left, bottom, right) on a page cut out at origin = (x0, y0) -> in
    the frame of the page it was cut from."""
    b = np.asarray(boxes, np.int32).reshape(-1, 4)
    arr = (_lib.TextCharC * max(len(b), 1))()
    for i, (t, l, bo, r) in enumerate(b.tolist()):
        arr[i] = _lib.TextCharC(0, t, l, bo, r)
    check(lib().ocrs_uncrop_chars(arr, C.c_size_t(len(b)), C.c_int(int(origin[0])), C.c_int(int(origin[1]))))
    return np.array([[arr[i].top, arr[i].left, arr[i].bottom, arr[i].right] for i in range(len(b))], np.int32).reshape(-1, 4)


def uncrop_lines(text_lines, origin):
    """recognize_text's output on a page cut out at origin = (x0, y0) -> new TextLines (None stays None) whose char boxes are
    in the frame of the page it was cut from (ocrs_uncrop_chars); text, log-probs and scores are kept."""
    out = []
    for t in text_lines:
        if t is None:
            out.append(None)
            continue
        boxes = uncrop_boxes([c.rect for c in t.chars()], origin)
        out.append(TextLine([TextChar(c.char, tuple(int(v) for v in b), c.logp) for c, b in zip(t.chars(), boxes)], t.score))
    return out


class Skew:
    """ocrs_engine_estimate_skew's outputs: angle (degrees; the page's content is turned counter-clockwise
    by it, deskew_map(.., angle) undoes it), scores (best coarse, runner-up coarse, at the angle), work_hw (the size the
    scores were taken at), coarse_index and fine_index (the best coarse angle and the estimate, in fine steps)."""
    __slots__ = ("angle", "scores", "work_hw", "coarse_index", "fine_index")

    def __repr__(self):
        return "Skew(angle=%r, scores=%r, work_hw=%r)" % (self.angle, self.scores, self.work_hw)


def _skew_struct(work_max_side=None, max_deg=None, coarse_step_deg=None, fine_step_deg=None):
    p = _lib.SkewParams()
    check(lib().ocrs_skew_params_default(C.byref(p)))
    if work_max_side is not None:
        p.work_max_side = int(work_max_side)
    if max_deg is not None:
        p.max_deg = float(max_deg)
    if coarse_step_deg is not None:
        p.coarse_step_deg = float(coarse_step_deg)
    if fine_step_deg is not None:
        p.fine_step_deg = float(fine_step_deg)
    return p


def skew_params(work_max_side=None, max_deg=None, coarse_step_deg=None, fine_step_deg=None):
    """ocrs_skew_params as a dict: ocrs_skew_params_default (work_max_side 1024, max_deg 15, coarse step 0.5,
    fine step 0.1) with the given fields replaced, checked by ocrs_skew_params_check (host only)."""
    p = _skew_struct(work_max_side, max_deg, coarse_step_deg, fine_step_deg)
    check(lib().ocrs_skew_params_check(C.byref(p)))
    return {"work_max_side": int(p.work_max_side), "max_deg": float(p.max_deg), "coarse_step_deg": float(p.coarse_step_deg),
            "fine_step_deg": float(p.fine_step_deg)}


def skew_table(first, n, step_deg):
    """ocrs_skew_table (host only): int32 [n, 2], the Q16 sine and cosine of the angles (first + i) * step_deg degrees."""
    t = np.zeros((int(n), 2), np.int32)
    check(lib().ocrs_skew_table(C.c_int(int(first)), C.c_size_t(int(n)), C.c_double(float(step_deg)), t.ctypes.data_as(C.POINTER(C.c_int32))))
    return t


def deskew_map(page_hw, angle_deg, expand=True):
    """ocrs_deskew_map (host only): the warp that undoes a skew of +angle_deg on a page_hw = (height, width) page ->
    ((out_h, out_w), m float32 [6]).  expand: the upright page holds the whole scan; else it keeps the scan's size."""
    hw = (C.c_int * 2)()
    m = np.zeros(6, np.float32)
    check(lib().ocrs_deskew_map(C.c_int(int(page_hw[0])), C.c_int(int(page_hw[1])), C.c_double(float(angle_deg)), C.c_int(1 if expand else 0),
                                hw, m.ctypes.data_as(C.POINTER(C.c_float))))
    return (int(hw[0]), int(hw[1])), m


def _map_arg(m):
    a = np.ascontiguousarray(m, np.float32).reshape(-1)
    if a.size != 6:
        raise ValueError("a map is six coefficients")
    return a


def unwarp_rects(rects, m):
    """ocrs_unwarp_rects (host only): word rects found on a page warped with m -> the same rects in the frame of the
    warp's source, float32 [n, 6] (a copy)."""
    a, mm = _rects_to_array(rects).copy(), _map_arg(m)
    check(lib().ocrs_unwarp_rects(a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(len(a)), mm.ctypes.data_as(C.POINTER(C.c_float))))
    return a


def unwarp_boxes(boxes, m):
    """ocrs_unwarp_chars on bare boxes: int32 [n, 4] (top, left, bottom, right) on a page warped with m -> in its source's frame."""
    b, mm = np.asarray(boxes, np.int32).reshape(-1, 4), _map_arg(m)
    arr = (_lib.TextCharC * max(len(b), 1))()
    for i, (t, l, bo, r) in enumerate(b.tolist()):
        arr[i] = _lib.TextCharC(0, t, l, bo, r)
    check(lib().ocrs_unwarp_chars(arr, C.c_size_t(len(b)), mm.ctypes.data_as(C.POINTER(C.c_float))))
    return np.array([[arr[i].top, arr[i].left, arr[i].bottom, arr[i].right] for i in range(len(b))], np.int32).reshape(-1, 4)


def unwarp_lines(text_lines, m):
    """recognize_text's output on a page warped with m -> new TextLines (None stays None) whose char boxes are in the frame
    of the warp's source (ocrs_unwarp_chars); text, log-probs and scores are kept."""
    out = []
    for t in text_lines:
        if t is None:
            out.append(None)
            continue
        boxes = unwarp_boxes([c.rect for c in t.chars()], m)
        out.append(TextLine([TextChar(c.char, tuple(int(v) for v in b), c.logp) for c, b in zip(t.chars(), boxes)], t.score))
    return out


class Outline:
    """ocrs_engine_find_outline's outputs: found, corners (float32 [4, 2]: TL, TR, BR, BL as (x, y) in the
    page's pixel-index frame; zeros when nothing was found), polarity (0: the sheet is lighter than the desk, 1: darker),
    counts and angles (of top, bottom, left, right: edge pixels, index into the angle table), work_hw (the size the peaks
    were taken at)."""
    __slots__ = ("found", "corners", "polarity", "counts", "angles", "work_hw")

    def __repr__(self):
        return "Outline(found=%r, corners=%r, polarity=%r, counts=%r)" % (self.found, self.corners.tolist(), self.polarity, self.counts)


def _outline_of(info):
    o = Outline()
    o.found, o.polarity = bool(info.found), int(info.polarity)
    o.corners = np.array(list(info.corners), np.float32).reshape(4, 2)
    o.counts, o.angles = tuple(int(v) for v in info.counts), tuple(int(v) for v in info.angles)
    o.work_hw = (int(info.work_h), int(info.work_w))
    return o


_OUTLINE_FIELDS = ("work_max_side", "max_deg", "step_deg", "min_step", "min_cover", "min_span", "min_area")


def _outline_struct(**params):
    p = _lib.OutlineParams()
    check(lib().ocrs_outline_params_default(C.byref(p)))
    for k, v in params.items():
        if k not in _OUTLINE_FIELDS:
            raise TypeError("outline: no parameter %r (one of %s)" % (k, ", ".join(_OUTLINE_FIELDS)))
        if v is not None:
            setattr(p, k, int(v) if k in ("work_max_side", "min_step") else float(v))
    return p


def outline_params(**params):
    """ocrs_outline_params as a dict: ocrs_outline_params_default (work_max_side 512, max_deg 15, step_deg
    0.5, min_step 8, min_cover 0.25, min_span 0.25, min_area 0.1) with the given fields replaced, checked by
    ocrs_outline_params_check (host only)."""
    p = _outline_struct(**params)
    check(lib().ocrs_outline_params_check(C.byref(p)))
    return {k: (int if k in ("work_max_side", "min_step") else float)(getattr(p, k)) for k in _OUTLINE_FIELDS}


def outline_choose(peaks, sc_table, work_hw, page_hw, **params):
    """ocrs_outline_choose (host only): the outline among the peaks (uint64 [2, 2, A, 16]: OcrEngine.edge_peaks) of a
    work_hw = (height, width) page taken from a page_hw page -> Outline."""
    t = np.ascontiguousarray(sc_table, np.int32).reshape(-1, 2)
    pk = np.ascontiguousarray(peaks, np.uint64).reshape(-1)
    if pk.size != 4 * len(t) * 16:
        raise ValueError("outline_choose: peaks are uint64 [2, 2, A, 16]")
    p, info = _outline_struct(**params), _lib.OutlineInfo()
    check(lib().ocrs_outline_choose(pk.ctypes.data_as(C.POINTER(C.c_uint64)), t.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(len(t)),
                                    C.c_int(int(work_hw[0])), C.c_int(int(work_hw[1])), C.c_int(int(page_hw[0])), C.c_int(int(page_hw[1])),
                                    C.byref(p), C.byref(info)))
    return _outline_of(info)


def page_corners(page_hw):
    """The outline of a page_hw = (height, width) page itself, float32 [4, 2]: quad_map of it is the identity map."""
    h, w = float(page_hw[0]), float(page_hw[1])
    return np.array([[-0.5, -0.5], [w - 0.5, -0.5], [w - 0.5, h - 0.5], [-0.5, h - 0.5]], np.float32)


def quad_map(corners):
    """ocrs_quad_map (host only): the projective map that shows the quad corners = TL, TR, BR, BL as (x, y) (the page's
    pixel-index frame) as an upright page -> ((out_h, out_w), m float32 [8])."""
    c = np.ascontiguousarray(corners, np.float32).reshape(-1)
    if c.size != 8:
        raise ValueError("a quad is four corners")
    hw = (C.c_int * 2)()
    m = np.zeros(8, np.float32)
    check(lib().ocrs_quad_map(c.ctypes.data_as(C.POINTER(C.c_float)), hw, m.ctypes.data_as(C.POINTER(C.c_float))))
    return (int(hw[0]), int(hw[1])), m


def _map8_arg(m):
    a = np.ascontiguousarray(m, np.float32).reshape(-1)
    if a.size != 8:
        raise ValueError("a projective map is eight coefficients")
    return a


def unproject_rects(rects, m):
    """ocrs_unproject_rects (host only): word rects found on a page projected with m -> the same rects in the frame of the
    projection's source, float32 [n, 6] (a copy)."""
    a, mm = _rects_to_array(rects).copy(), _map8_arg(m)
    check(lib().ocrs_unproject_rects(a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(len(a)), mm.ctypes.data_as(C.POINTER(C.c_float))))
    return a


def unproject_boxes(boxes, m):
    """ocrs_unproject_chars on bare boxes: int32 [n, 4] (top, left, bottom, right) on a page projected with m -> in its source's frame."""
    b, mm = np.asarray(boxes, np.int32).reshape(-1, 4), _map8_arg(m)
    arr = (_lib.TextCharC * max(len(b), 1))()
    for i, (t, l, bo, r) in enumerate(b.tolist()):
        arr[i] = _lib.TextCharC(0, t, l, bo, r)
    check(lib().ocrs_unproject_chars(arr, C.c_size_t(len(b)), mm.ctypes.data_as(C.POINTER(C.c_float))))
    return np.array([[arr[i].top, arr[i].left, arr[i].bottom, arr[i].right] for i in range(len(b))], np.int32).reshape(-1, 4)


def unproject_lines(text_lines, m):
    """recognize_text's output on a page projected with m -> new TextLines (None stays None) whose char boxes are in the
    frame of the projection's source (ocrs_unproject_chars); text, log-probs and scores are kept."""
    out = []
    for t in text_lines:
        if t is None:
            out.append(None)
            continue
        boxes = unproject_boxes([c.rect for c in t.chars()], m)
        out.append(TextLine([TextChar(c.char, tuple(int(v) for v in b), c.logp) for c, b in zip(t.chars(), boxes)], t.score))
    return out


def _work_hw(work_size):
    """None = the page's own size (0, 0)."""
    return (0, 0) if work_size is None else (int(work_size[0]), int(work_size[1]))


def _detect_words_batch(name, handle, inputs, scores, tiled=False, work_sizes=None, work_filter="auto"):
    """ocrs_{engine,group}_detect_words_batch[_at | _tiled | _scored] (name without the suffix; _at when work sizes are
    given, else _tiled when tiled, else _scored when scored) -> rects per page [, score per page, pixels per page]."""
    n = len(inputs)
    if work_sizes is not None and len(work_sizes) != n:
        raise ValueError("detect_words_batch: one work size per page")
    pages = _page_array(inputs)
    rects = C.POINTER(C.c_float)()
    offs = (C.c_size_t * (n + 1))()
    overlap = _tile_overlap(tiled)
    sc, px = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
    out = (C.byref(rects), offs, C.byref(sc) if scores else None, C.byref(px) if scores else None)
    if work_sizes is not None:
        hw = (C.c_int * (2 * n))(*[v for s in work_sizes for v in _work_hw(s)])
        check(getattr(lib(), name + "_at")(handle, pages, C.c_size_t(n), hw, C.c_int(_lib.RESAMPLE_FILTERS[work_filter]),
                                           C.c_int(0 if overlap is None else 1), C.c_int(-1 if overlap is None else overlap), *out))
    elif overlap is not None:
        check(getattr(lib(), name + "_tiled")(handle, pages, C.c_size_t(n), C.c_int(overlap), *out))
    elif scores:
        check(getattr(lib(), name + "_scored")(handle, pages, C.c_size_t(n), *out))
    else:
        check(getattr(lib(), name)(handle, pages, C.c_size_t(n), *out[:2]))
    total = offs[n]
    flat = _take_rects(rects, total)
    words = [flat[offs[i]:offs[i + 1]] for i in range(n)]
    if not scores:
        return words
    fs, fp = _take(sc, total, np.float32), _take(px, total, np.uint32)
    return words, [fs[offs[i]:offs[i + 1]] for i in range(n)], [fp[offs[i]:offs[i + 1]] for i in range(n)]


def _pack_lines(lines):
    offs = [0]
    flat = []
    for l in lines:
        a = _rects_to_array(l)
        flat.append(a)
        offs.append(offs[-1] + len(a))
    rects = np.concatenate(flat) if flat else np.zeros((0, 6), np.float32)
    return np.ascontiguousarray(rects, np.float32), np.array(offs, dtype=np.uintp)


class OcrEngine:
    """lib.rs:111-301.  Word rects are rows of 6 floats
    (center.x, center.y, up.x, up.y, width, height)."""

    def __init__(self, params=None, **kw):
        params = params or OcrEngineParams(**kw)
        self._params = params
        p = _lib.EngineParams()
        p.detection_model = params.detection_model._h if params.detection_model else None
        p.recognition_model = params.recognition_model._h if params.recognition_model else None
        p.debug = 1 if params.debug else 0
        p.decode_method = 0 if params.decode_method[0] == "greedy" else 1
        p.beam_width = params.decode_method[1]
        p.alphabet = params.alphabet.encode("utf-8") if params.alphabet is not None else None
        p.allowed_chars = params.allowed_chars.encode("utf-8") if params.allowed_chars is not None else None
        p.numerics = NUMERICS[params.numerics]
        p.coalesce = int(params.coalesce)
        p.coalesce_pages = int(params.coalesce_pages)
        p.coalesce_window_us = int(params.coalesce_window_us)
        p.layout_threads = int(params.layout_threads)
        p.rec_max_pixels = int(params.rec_max_pixels)
        self._h = C.c_void_p()
        check(lib().ocrs_engine_new(C.byref(p), C.byref(self._h)))
        for k, v in params.options.items():
            self.set_option(k, v)

    def set_option(self, name, value):
        """ocrs_engine_set_option: this engine's copy of a tuning option (results never depend on one)."""
        check(lib().ocrs_engine_set_option(self._h, name.encode(), C.c_long(int(value))))

    def get_option(self, name):
        v = C.c_long(0)
        check(lib().ocrs_engine_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    @classmethod
    def _borrowed(cls, handle, keep):
        """An engine owned by somebody else (an EngineGroup member): same methods, never freed here."""
        self = cls.__new__(cls)
        self._params = None
        self._h = handle
        self._keep = keep
        self._owned = False
        return self

    def device(self):
        d = C.c_int(-1)
        check(lib().ocrs_engine_device(self._h, C.byref(d)))
        return d.value

    def coalesce_stats(self):
        """{stage: (merged batches run, caller requests they carried)} — ocrs_engine_coalesce_stats."""
        det, rec = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        check(lib().ocrs_engine_coalesce_stats(self._h, det, rec))
        return {"detect": (int(det[0]), int(det[1])), "recognize": (int(rec[0]), int(rec[1]))}

    # ---- lib.rs:183-187
    def prepare_input(self, image):
        a = np.ascontiguousarray(image.data)
        if image.order == DimOrder.Hwc:
            h, w, c = a.shape
        else:
            c, h, w = a.shape
        h_out = C.c_void_p()
        check(lib().ocrs_engine_prepare_input(self._h, a.ctypes.data_as(C.c_void_p), 0 if a.dtype == np.uint8 else 1,
                                              image.order, h, w, c, C.byref(h_out)))
        return OcrInput(h_out)

    def input_from_grey(self, grey):
        """ocrs_engine_page_from_grey: a page from an already prepared grey image ([H, W] or [1, H, W] float32, what
        OcrInput.image() returns), copied bit for bit."""
        a = np.ascontiguousarray(grey, np.float32)
        a = a.reshape(a.shape[-2], a.shape[-1])
        h_out = C.c_void_p()
        check(lib().ocrs_engine_page_from_grey(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0], a.shape[1], C.byref(h_out)))
        return OcrInput(h_out)

    def prepare_input_batch_raw(self, host_ptrs, dtype, order, h, w, c):
        """n equally sized host images given as raw pointers (e.g. pinned buffers from ocrs_host_malloc): one call,
        one wait."""
        n = len(host_ptrs)
        arr = (C.c_void_p * n)(*host_ptrs)
        out = (C.c_void_p * n)()
        check(lib().ocrs_engine_prepare_input_batch(self._h, arr, C.c_size_t(n), 0 if dtype == np.uint8 else 1, order,
                                                    h, w, c, out))
        return _new_inputs(out, n)

    def prepare_input_device(self, d_ptr, dtype, order, h, w, c):
        """Pixels already in HBM (a raw device pointer), e.g. from bench.py."""
        h_out = C.c_void_p()
        check(lib().ocrs_engine_prepare_input_device(self._h, C.c_void_p(d_ptr), 0 if dtype == np.uint8 else 1, order,
                                                     h, w, c, C.byref(h_out)))
        return OcrInput(h_out)

    def prepare_input_jpeg(self, data):
        """prepare_input fed with a JPEG file's bytes (ocrs-cli/src/main.rs:312-333 decodes on the host first): Huffman
        decoding on the host, IDCT / upsampling / colour conversion / grey conversion on the GPU.  -> (OcrInput, bytes that
        crossed PCIe).  Raises OcrsError (IMAGE_SOURCE) for flavours the hand-off does not cover."""
        h_out = C.c_void_p()
        cb = C.c_size_t(0)
        buf = C.create_string_buffer(bytes(data), len(data))
        check(lib().ocrs_engine_prepare_input_jpeg(self._h, buf, C.c_size_t(len(data)), C.byref(h_out), C.byref(cb)))
        return OcrInput(h_out), cb.value

    # ---- quarter turns and auto-orientation
    def rotate(self, inp, k):
        """ocrs_engine_rotate_page: np.rot90(page, k) (counter-clockwise, any integer k) as a new resident page."""
        return self.rotate_batch([inp], [k])[0]

    def rotate_batch(self, inputs, ks):
        """ocrs_engine_rotate_pages: pages of any sizes, each by its own k, in one launch."""
        n = len(inputs)
        if len(ks) != n:
            raise ValueError("rotate_batch: one k per page")
        pages = _page_array(inputs)
        turns = (C.c_int * n)(*[int(k) for k in ks])
        out = (C.c_void_p * n)()
        check(lib().ocrs_engine_rotate_pages(self._h, pages, C.c_size_t(n), turns, out))
        return _new_inputs(out, n)

    def detect_orientation(self, inp, max_lines=8):
        """ocrs_engine_detect_orientation -> Orientation: which quarter turn makes the page read (rotate(inp,
        result.quarter_turns) is the upright page).  max_lines: lines recognised per candidate turn (0 = all)."""
        o = Orientation()
        k = C.c_int(0)
        o.vote, o.scores, o.n_chars = np.zeros(2, np.float64), np.zeros(4, np.float64), np.zeros(4, np.uint32)
        check(lib().ocrs_engine_detect_orientation(self._h, inp._h, C.c_size_t(int(max_lines)), C.byref(k),
                                                   o.vote.ctypes.data_as(C.POINTER(C.c_double)),
                                                   o.scores.ctypes.data_as(C.POINTER(C.c_double)),
                                                   o.n_chars.ctypes.data_as(C.POINTER(C.c_uint32))))
        o.quarter_turns = k.value
        return o

    # ---- the page operations with parameters per page
    @staticmethod
    def _page_op_args(name, params_cls, struct_of, inputs, params):
        """The pages of `inputs` and their parameter structs, as arrays: page i with struct_of(**params[i]) (a dict of
        keywords, or None for the default; `params` is one for all, or one per page)."""
        n = len(inputs)
        if params is None or isinstance(params, dict):
            params = [params] * n
        if len(params) != n:
            raise ValueError("%s_batch: one parameter set per page" % name)
        return _page_array(inputs), (params_cls * n)(*[struct_of(**(p or {})) for p in params])

    def _page_op_batch(self, name, entry, params_cls, struct_of, info_cls, inputs, params, mask, info):
        """<name>_batch: `entry` on the pages of `inputs`, page i with the params struct struct_of(**params[i]) (a dict of
        keywords, or None for the default; `params` is one for all, or one per page).  mask: None for an entry point that
        takes no masks.  -> pages, or (pages[, masks][, infos])."""
        n = len(inputs)
        pages, ps = self._page_op_args(name, params_cls, struct_of, inputs, params)
        out = (C.c_void_p * n)()
        masks = (C.POINTER(C.c_uint8) * n)()
        infos = (info_cls * n)()
        outputs = ([] if mask is None else [masks if mask else None]) + [infos if info else None]
        check(entry(self._h, pages, C.c_size_t(n), ps, out, *outputs))
        made = _new_inputs(out, n)
        res = [made]
        if mask:
            got = []
            for i in range(n):
                h, w = made[i].shape[-2:]
                got.append(np.ctypeslib.as_array(masks[i], shape=(h * w,)).reshape(h, w).copy())
                lib().ocrs_buffer_free(masks[i])
            res.append(got)
        if info:
            res.append([infos[i].as_dict() for i in range(n)])
        return tuple(res) if mask or info else made

    # ---- page normalisation
    def normalize(self, inp, tile=64, polarity="auto", flatten=True, levels=True, info=False):
        """ocrs_engine_normalize_page: the page with its background flattened, its levels stretched and its polarity made
        dark-on-light, as a new resident page of the same size (ink -0.5, paper +0.5).  tile: a power of two, 16 .. 256;
        polarity: "auto" (a per-tile vote), "keep" or "invert".  info=True: -> (page, {"dark", "vote", "white", "lo", "hi",
        "counted"})."""
        out = self.normalize_batch([inp], [{"tile": tile, "polarity": polarity, "flatten": flatten, "levels": levels}], info=info)
        return (out[0][0], out[1][0]) if info else out[0]

    def normalize_batch(self, inputs, params=None, info=False):
        """ocrs_engine_normalize_pages: pages of any sizes, each with its own parameters (a dict of normalize's keywords, or
        None for the default; one for all, or one per page), all passes for the whole batch on one stream.  info=True: ->
        (pages, infos)."""
        return self._page_op_batch("normalize", lib().ocrs_engine_normalize_pages, _lib.NormalizeParams, _normalize_struct, _lib.NormalizeInfo,
                                           inputs, params, None, info)

    # ---- ruled-line removal
    def remove_rules(self, inp, min_length=96, max_thickness=8, margin=1, threshold=0.0, paper=None, mask=False, info=False):
        """ocrs_engine_remove_rules_page: the page with its long thin rules (table grids, form lines, underlines) overwritten
        by the paper's level, as a new resident page of the same size; every other pixel keeps its bits.  The page is dark ink
        on light paper (normalize makes it so) with axis-aligned rules (deskew first).  A rule: ink (< threshold) in a run of
        at least min_length pixels, at most max_thickness thick; margin: the rows and columns of half-tone edge taken with it;
        paper: the fill, None = the page's median paper level.  A stroke that crosses a rule is kept.  mask=True: also the
        uint8 [H, W] mask (bit 0 horizontal rule, 1 vertical rule, 2 margin, 3 kept crossing); info=True: also {"paper_bin",
        "fill", "ink", "counted", "h_removed", "v_removed", "overwritten", "kept"}.  -> page, or (page[, mask][, info])."""
        out = self.remove_rules_batch([inp], [{"min_length": min_length, "max_thickness": max_thickness, "margin": margin,
                                               "threshold": threshold, "paper": paper}], mask=mask, info=info)
        return tuple(o[0] for o in out) if mask or info else out[0]

    def remove_rules_batch(self, inputs, params=None, mask=False, info=False):
        """ocrs_engine_remove_rules_pages: pages of any sizes, each with its own parameters (a dict of remove_rules's keywords,
        or None for the default; one for all, or one per page), all passes for the whole batch on one stream.  -> pages, or
        (pages[, masks][, infos])."""
        return self._page_op_batch("remove_rules", lib().ocrs_engine_remove_rules_pages, _lib.RulesParams, _rules_struct, _lib.RulesInfo,
                                           inputs, params, mask, info)

    # ---- despeckling
    def despeckle(self, inp, max_area=4, max_hole=0, keep_near=0, threshold=0.0, paper=None, ink_level=None, mask=False, info=False):
        """ocrs_engine_despeckle_page: the page with its isolated specks overwritten by the paper's level and its pinholes by
        the ink's, as a new resident page of the same size; every other pixel keeps its bits.  The page is dark ink on light
        paper (normalize makes it so).  A speck: an 8-connected component of ink (< threshold) of at most max_area pixels;
        keep_near > 0: one with a pixel within that Chebyshev distance of larger ink is kept (i-dots, full stops).  A hole: a
        4-connected component of everything else of at most max_hole pixels (0, the default: none is filled).  paper,
        ink_level: the fills, None = the page's median paper and ink levels.  mask=True: also the uint8 [H, W] mask (bit 0
        speck, 1 hole, 2 kept); info=True: also {"paper_bin", "ink_bin", "paper_fill", "ink_fill", "ink", "counted", "specks",
        "kept", "speck_pixels", "kept_pixels", "holes", "hole_pixels"}.  -> page, or (page[, mask][, info])."""
        out = self.despeckle_batch([inp], [{"max_area": max_area, "max_hole": max_hole, "keep_near": keep_near, "threshold": threshold,
                                            "paper": paper, "ink_level": ink_level}], mask=mask, info=info)
        return tuple(o[0] for o in out) if mask or info else out[0]

    def despeckle_batch(self, inputs, params=None, mask=False, info=False):
        """ocrs_engine_despeckle_pages: pages of any sizes, each with its own parameters (a dict of despeckle's keywords, or
        None for the default; one for all, or one per page), all passes for the whole batch on one stream.  -> pages, or
        (pages[, masks][, infos])."""
        return self._page_op_batch("despeckle", lib().ocrs_engine_despeckle_pages, _lib.SpeckleParams, _speckle_struct, _lib.SpeckleInfo,
                                           inputs, params, mask, info)

    # ---- adaptive binarisation
    def binarize(self, inp, radius=15, k=0.34, keep_ink=False, ink_level=None, paper=None, mask=False, info=False):
        """ocrs_engine_binarize_page: the page cut into ink and paper by Sauvola's local threshold, in exact integers, as a
        new resident page of the same size.  The page is dark ink on light paper (normalize makes it so).  A pixel is ink
        when its bin lies under m (1 + k (s / 128 - 1)), m and s the mean and the standard deviation of the bins in the
        (2 radius + 1)^2 window around it, clipped to the page; k is rounded to 1/256 (0: the plain local mean).  A flat
        window has no ink: a blank page comes back as paper, and so does an all-black one.  Ink is written as ink_level
        (None: -0.5) or, with keep_ink, keeps its own bits; every other pixel is written as paper (None: +0.5); NaN pixels
        keep their bits.  mask=True: also the uint8 [H, W] mask (bit 0 ink); info=True: also {"counted", "ink",
        "ink_fill", "paper_fill"}.  -> page, or (page[, mask][, info])."""
        out = self.binarize_batch([inp], [{"radius": radius, "k": k, "keep_ink": keep_ink, "ink_level": ink_level, "paper": paper}],
                                  mask=mask, info=info)
        return tuple(o[0] for o in out) if mask or info else out[0]

    def binarize_batch(self, inputs, params=None, mask=False, info=False):
        """ocrs_engine_binarize_pages: pages of any sizes, each with its own parameters (a dict of binarize's keywords, or
        None for the default; one for all, or one per page), all passes for the whole batch on one stream.  -> pages, or
        (pages[, masks][, infos])."""
        return self._page_op_batch("binarize", lib().ocrs_engine_binarize_pages, _lib.BinarizeParams, _binarize_struct, _lib.BinarizeInfo,
                                           inputs, params, mask, info)

    # ---- stroke repair
    def morph(self, inp, op="close", rx=1, ry=None, mask=False, info=False):
        """ocrs_engine_morph_page: the page with its ink thickened, thinned, closed or opened by running minima and maxima
        over the window of 2 ry + 1 rows of 2 rx + 1 pixels around every pixel, clipped to the page, as a new resident page
        of the same size (ry=None: ry = rx; 0 .. 63, not both 0).  The page is dark ink on light paper (normalize makes it
        so).  "thicken": the darkest pixel of the window (ink grows); "thin": the lightest (ink shrinks); "close": thicken
        then thin (gaps and breaks in the ink narrower than the window are bridged, everything else keeps its extent);
        "open": thin then thicken (hairs and bridges of ink narrower than the window vanish, fused characters separate).
        Every result pixel has the bits of some source pixel; NaN pixels are not counted and keep their bits.  mask=True:
        also the uint8 [H, W] mask (bit 0 ink after, bit 1 changed); info=True: also {"counted", "changed", "ink_before",
        "ink_after"}.  -> page, or (page[, mask][, info])."""
        out = self.morph_batch([inp], [{"op": op, "rx": rx, "ry": ry}], mask=mask, info=info)
        return tuple(o[0] for o in out) if mask or info else out[0]

    def morph_batch(self, inputs, params=None, mask=False, info=False):
        """ocrs_engine_morph_pages: pages of any sizes, each with its own parameters (a dict of morph's keywords, or None
        for the default; one for all, or one per page; ops and radii mix freely), all passes for the whole batch on one
        stream.  -> pages, or (pages[, masks][, infos])."""
        return self._page_op_batch("morph", lib().ocrs_engine_morph_pages, _lib.MorphParams, _morph_struct, _lib.MorphInfo,
                                           inputs, params, mask, info)

    # ---- grain removal
    def rank(self, inp, rx=1, ry=None, percent=50, tail=20, mask=False, info=False):
        """ocrs_engine_rank_page: the page with its grain removed by a rank filter over the window of 2 ry + 1 rows of
        2 rx + 1 pixels around every pixel, clipped to the page, as a new resident page of the same size (ry=None: ry = rx;
        0 .. 7, not both 0).  percent: the rank taken among the n counted pixels of the window, (percent (n - 1) + 50) // 100
        from the darkest: 50 the median, 0 the darkest (morph's "thicken"), 100 the lightest ("thin").  tail: 0 filters
        every pixel; 1 .. 50 filters outliers only: a pixel whose own ranks in its window meet [tail, 100 - tail] percent
        keeps its bits, which is what keeps hairlines and small print.  Every result pixel has the bits of some source
        pixel; NaN pixels are not counted and keep their bits.  It belongs before binarize.  mask=True: also the uint8
        [H, W] mask (bit 0 ink after, bit 1 changed); info=True: also {"counted", "changed", "ink_before", "ink_after",
        "spared"}.  -> page, or (page[, mask][, info])."""
        out = self.rank_batch([inp], [{"rx": rx, "ry": ry, "percent": percent, "tail": tail}], mask=mask, info=info)
        return tuple(o[0] for o in out) if mask or info else out[0]

    def rank_batch(self, inputs, params=None, mask=False, info=False):
        """ocrs_engine_rank_pages: pages of any sizes, each with its own parameters (a dict of rank's keywords, or None
        for the default; one for all, or one per page; radii, percents and tails mix freely), at most three launches for the
        whole batch on one stream.  -> pages, or (pages[, masks][, infos])."""
        return self._page_op_batch("rank", lib().ocrs_engine_rank_pages, _lib.RankParams, _rank_struct, _lib.RankInfo,
                                           inputs, params, mask, info)

    # ---- page framing
    def clean_frame(self, inp, depth=128, sides=15, min_area=0, threshold=0.0, paper=None, mask=False, info=False):
        """ocrs_engine_clean_frame_page: the page with the ink that is connected to its frame (scanner bars, the wedge of a
        skewed sheet, the slice of a neighbouring page, a gutter shadow) overwritten by the paper's level, as a new resident
        page of the same size; every other pixel keeps its bits.  The page is dark ink on light paper (normalize makes it
        so).  Only ink (< threshold) within `depth` pixels of the nearest side is looked at (0: the whole page), as
        8-connected components inside that ring; a component with a pixel on one of `sides` (bits 0 left, 1 top, 2 right, 3
        bottom, or letters out of "LTRB") and at least min_area pixels is removed, a smaller one is kept.  paper: the fill,
        None = the page's median paper level.  mask=True: also the uint8 [H, W] mask (bit 0 removed, 1 kept, 2 ink in the
        ring); info=True: also {"paper_bin", "paper_fill", "ink", "counted", "ring_ink", "removed", "removed_pixels", "kept",
        "kept_pixels"}.  -> page, or (page[, mask][, info])."""
        out = self.clean_frame_batch([inp], [{"depth": depth, "sides": sides, "min_area": min_area, "threshold": threshold, "paper": paper}],
                                     mask=mask, info=info)
        return tuple(o[0] for o in out) if mask or info else out[0]

    def clean_frame_batch(self, inputs, params=None, mask=False, info=False):
        """ocrs_engine_clean_frame_pages: pages of any sizes, each with its own parameters (a dict of clean_frame's keywords,
        or None for the default; one for all, or one per page), all passes for the whole batch on one stream.  -> pages, or
        (pages[, masks][, infos])."""
        return self._page_op_batch("clean_frame", lib().ocrs_engine_clean_frame_pages, _lib.FrameParams, _frame_struct, _lib.FrameInfo,
                                           inputs, params, mask, info)

    def ink_profiles(self, inp, threshold=0.0, cols=True, rows=True):
        """ocrs_engine_ink_profiles: the pixels under `threshold` per column (uint32 [W]) and per row (uint32 [H]) ->
        (col_ink, row_ink); cols=False or rows=False: None in its place, and the library is not asked for it."""
        h, w = inp.shape[-2:]
        c = np.zeros(w, np.uint32) if cols else None
        r = np.zeros(h, np.uint32) if rows else None
        check(lib().ocrs_engine_ink_profiles(self._h, inp._h, C.c_float(float(threshold)),
                                             c.ctypes.data_as(C.POINTER(C.c_uint32)) if cols else None,
                                             r.ctypes.data_as(C.POINTER(C.c_uint32)) if rows else None))
        return c, r

    # ---- page measurement
    def measure(self, inp, threshold=0.0, min_area=4):
        """ocrs_engine_measure_page: the page's run-length and component histograms -> {"ink", "components", "counted"
        (ints), "run_h", "run_v", "comp_h", "comp_w" (uint32 [256]), "area_by_h" (uint64 [256])}: exact integers, equal to
        tests/measure_ref.py in every bin.  Ink is v < threshold; a component of fewer than min_area pixels (0 .. 65535) is
        not counted.  The page is not changed and none is made."""
        return self.measure_batch([inp], [{"threshold": threshold, "min_area": min_area}])[0]

    def measure_batch(self, inputs, params=None):
        """ocrs_engine_measure_pages: pages of any sizes, each with its own parameters (a dict of measure's keywords, or
        None for the default; one for all, or one per page), all passes for the whole batch on one stream -> infos."""
        n = len(inputs)
        pages, ps = self._page_op_args("measure", _lib.MeasureParams, _measure_struct, inputs, params)
        infos = (_lib.MeasureInfo * n)()
        check(lib().ocrs_engine_measure_pages(self._h, pages, C.c_size_t(n), ps, infos))
        return [infos[i].as_dict() for i in range(n)]

    # ---- reverse-video repair
    def unreverse(self, inp, min_height=32, min_width=64, min_fill=0.4, min_holes=3, max_hole=0, threshold=0.0, mask=False, info=False):
        """ocrs_engine_unreverse_page: the page with its solid dark panels that enclose light marks (a table's header band, a
        screenshot's buttons and sidebars, a dark code pane), and what they enclose, inverted by flipping the sign bit, as a
        new resident page of the same size; every other pixel keeps its bits.  A candidate: an 8-connected component of ink
        (< threshold) whose box is at least min_height x min_width and which fills at least min_fill of it.  A hole: a
        4-connected component of everything outside the candidates that does not touch the page's edge; it counts when
        max_hole is 0 or it has at most max_hole pixels.  A candidate that encloses at least min_holes counting holes is a
        panel.  The five defaults are uncalibrated.  mask=True: also the uint8 [H, W] mask (bit 0 inverted, 1 candidate, 2
        panel, 3 hole); info=True: also {"ink", "components", "candidates", "panels", "panel_pixels", "holes", "hole_pixels",
        "skipped_holes", "inverted"}.  -> page, or (page[, mask][, info])."""
        out = self.unreverse_batch([inp], [{"min_height": min_height, "min_width": min_width, "min_fill": min_fill, "min_holes": min_holes,
                                            "max_hole": max_hole, "threshold": threshold}], mask=mask, info=info)
        return tuple(o[0] for o in out) if mask or info else out[0]

    def unreverse_batch(self, inputs, params=None, mask=False, info=False):
        """ocrs_engine_unreverse_pages: pages of any sizes, each with its own parameters (a dict of unreverse's keywords, or
        None for the default; one for all, or one per page), all passes for the whole batch on one stream.  -> pages, or
        (pages[, masks][, infos])."""
        return self._page_op_batch("unreverse", lib().ocrs_engine_unreverse_pages, _lib.ReverseParams, _reverse_struct, _lib.ReverseInfo,
                                           inputs, params, mask, info)

    def text_scale(self, inp, min_height_strokes=None, **kw):
        """measure (keywords threshold, min_area) followed by measure_choose -> TextScale."""
        return measure_choose(self.measure(inp, **kw), min_height_strokes)

    def _work_size_for_text(self, inp, target_height=True, **kw):
        """The work size at which the page's text is target_height pixels tall (True: WORK_TEXT_HEIGHT_DEFAULT): text_scale
        (its keywords in kw), work_scale_for_text within [1/8, 4], work_size.  A blank page keeps its size."""
        target = None if target_height is True else target_height
        return work_size(inp.shape[-2:], scale=work_scale_for_text(self.text_scale(inp, **kw).text_height, target))

    def crop(self, inp, rect, fill=0.5):
        """ocrs_engine_crop_page: rect = (x0, y0, x1, y1), half open, cut out of the page as a new resident page of (y1 - y0)
        x (x1 - x0), each 1 .. 65535.  The rectangle may reach outside the page: a pixel there is `fill` (a float32 scalar
        keeps its bits, NaN payloads included)."""
        return self.crop_batch([inp], [rect], [fill])[0]

    def crop_batch(self, inputs, rects, fill=0.5):
        """ocrs_engine_crop_pages: pages of any sizes, each with its own rectangle and fill (one fill for all, or one per
        page), in one launch."""
        n = len(inputs)
        if len(rects) != n:
            raise ValueError("crop_batch: one rectangle per page")
        fills = list(fill) if isinstance(fill, (list, tuple, np.ndarray)) else [fill] * n
        if len(fills) != n:
            raise ValueError("crop_batch: one fill per page")
        words = np.zeros(max(n, 1), np.float32)
        for i, f in enumerate(fills):   # a float32 by its word: a conversion could quiet a signalling NaN
            words.view(np.uint32)[i] = f.view(np.uint32) if isinstance(f, np.float32) else np.array([f], np.float32).view(np.uint32)[0]
        rs = (_lib.CropRect * max(n, 1))(*[_lib.CropRect(*[int(v) for v in r]) for r in rects])
        out = (C.c_void_p * n)()
        check(lib().ocrs_engine_crop_pages(self._h, _page_array(inputs), C.c_size_t(n), rs, words.ctypes.data_as(C.POINTER(C.c_float)), out))
        return _new_inputs(out, n)

    def _framed(self, inp, kw):
        """clean_frame, ink_profiles of the cleaned page and frame_choose, each with its own keywords out of kw ->
        (cleaned page, frame info, choice)."""
        kw = dict(kw)
        clean_kw = {k: kw.pop(k) for k in ("depth", "sides", "min_area", "threshold", "paper") if k in kw}
        choice_kw = {k: kw.pop(k) for k in ("min_count", "pad", "gutter_min_width", "gutter_max_ink") if k in kw}
        if kw:
            raise TypeError("unexpected keywords: %s" % ", ".join(sorted(kw)))
        page, info = self.clean_frame(inp, info=True, **clean_kw)
        cols, rows = self.ink_profiles(page, clean_kw.get("threshold", 0.0))
        return page, info, frame_choose(page.shape[-2:], cols, rows, **choice_kw)

    def frame(self, inp, info=False, **kw):
        """The page without what surrounds its text: clean_frame, then ink_profiles of the cleaned page, then frame_choose,
        then crop to the content box.  Keywords: clean_frame's (depth, sides, min_area, threshold, paper) and frame_choose's
        (min_count, pad).  -> (page, (x0, y0)[, info]): the origin of the new page on the old one, for uncrop_rects /
        uncrop_lines; info=True: also clean_frame's info with the choice under "choice".  A page without ink comes back whole."""
        page, finfo, c = self._framed(inp, kw)
        out = self.crop(page, (c["x0"], c["y0"], c["x1"], c["y1"]), np.float32(finfo["paper_fill"]))
        return (out, (c["x0"], c["y0"]), dict(finfo, choice=c)) if info else (out, (c["x0"], c["y0"]))

    def split_spread(self, inp, info=False, **kw):
        """The pages of a spread: clean_frame, ink_profiles, frame_choose, then the content box cut at the gutter ->
        [(page, (x0, y0))], one entry without a gutter, otherwise the left page [x0, gutter_x) first and the right page
        [gutter_x, x1) second.  Keywords: clean_frame's and frame_choose's (gutter_min_width and gutter_max_ink too).
        info=True: -> (that list, clean_frame's info with the choice under "choice")."""
        page, finfo, c = self._framed(inp, kw)
        cuts = [c["x0"], c["gutter_x"], c["x1"]] if c["x0"] < c["gutter_x"] < c["x1"] else [c["x0"], c["x1"]]   # no empty page
        rects = [(a, c["y0"], b, c["y1"]) for a, b in zip(cuts[:-1], cuts[1:])]
        made = self.crop_batch([page] * len(rects), rects, np.float32(finfo["paper_fill"]))
        parts = [(p, (r[0], r[1])) for p, r in zip(made, rects)]
        return (parts, dict(finfo, choice=c)) if info else parts

    # ---- page deskew
    def skew_scores(self, inputs, sc_table):
        """ocrs_engine_skew_scores: the skew profile scores of pages of any sizes (a side at most 4096) at the angles of
        sc_table (int32 [A, 2], Q16 sine and cosine: skew_table) -> uint64 [n, A], in one launch."""
        n = len(inputs)
        t = np.ascontiguousarray(sc_table, np.int32).reshape(-1, 2)
        out = np.zeros((n, len(t)), np.uint64)
        check(lib().ocrs_engine_skew_scores(self._h, _page_array(inputs), C.c_size_t(n), t.ctypes.data_as(C.POINTER(C.c_int32)),
                                            C.c_size_t(len(t)), out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def estimate_skew(self, inp, work_max_side=None, max_deg=None, coarse_step_deg=None, fine_step_deg=None):
        """ocrs_engine_estimate_skew -> Skew: the angle the page's content is turned by, counter-clockwise, in degrees
        (defaults: searched within +-15 in steps of 0.5, then 0.1, on a copy of at most 1024 pixels a side)."""
        p = _skew_struct(work_max_side, max_deg, coarse_step_deg, fine_step_deg)
        info = _lib.SkewInfo()
        check(lib().ocrs_engine_estimate_skew(self._h, inp._h, C.byref(p), C.byref(info)))
        s = Skew()
        s.angle, s.scores, s.work_hw = float(info.angle_deg), (int(info.best_score), int(info.second_score), int(info.fine_score)), (int(info.work_h), int(info.work_w))
        s.coarse_index, s.fine_index = int(info.coarse_index), int(info.fine_index)
        return s

    def warp(self, inp, m, out_hw, fill=0.5):
        """ocrs_engine_warp_page: the page seen through the affine map m (six coefficients: output pixel -> page position)
        as a new resident page of out_hw = (height, width); a tap outside the page is `fill`."""
        return self.warp_batch([inp], [m], [out_hw], [fill])[0]

    def warp_batch(self, inputs, ms, out_hws, fills=0.5):
        """ocrs_engine_warp_pages: pages of any sizes, each with its own map, size and fill (or one fill for all), in one
        launch."""
        n = len(inputs)
        if not isinstance(fills, (list, tuple, np.ndarray)):
            fills = [fills] * n
        if len(ms) != n or len(out_hws) != n or len(fills) != n:
            raise ValueError("warp_batch: one map, one size and one fill per page")
        mm = np.ascontiguousarray(np.concatenate([_map_arg(m) for m in ms]) if n else np.zeros(0), np.float32)
        hw = (C.c_int * (2 * n))(*[int(v) for s in out_hws for v in (s[0], s[1])])
        fl = np.ascontiguousarray(np.asarray(fills, np.float32).reshape(-1))
        out = (C.c_void_p * n)()
        check(lib().ocrs_engine_warp_pages(self._h, _page_array(inputs), C.c_size_t(n), hw, mm.ctypes.data_as(C.POINTER(C.c_float)),
                                           fl.ctypes.data_as(C.POINTER(C.c_float)), out))
        return _new_inputs(out, n)

    def deskew(self, inp, angle=None, expand=True, fill=0.5, min_deg=0.2):
        """The upright page -> (page, m, angle).  angle: the skew in degrees (None: what estimate_skew finds).  m is the
        map of the warp (deskew_map): unwarp_rects / unwarp_lines with it bring results back to inp's frame.  An |angle|
        below min_deg leaves the page alone: inp itself comes back, with the identity map."""
        if angle is None:
            angle = self.estimate_skew(inp).angle
        angle = float(angle)
        hw = inp.shape[-2:]
        if abs(angle) < min_deg:
            return inp, deskew_map(hw, 0.0, expand=False)[1], angle
        out_hw, m = deskew_map(hw, angle, expand=expand)
        return self.warp(inp, m, out_hw, fill=fill), m, angle

    # ---- perspective correction
    def edge_peaks(self, inputs, sc_table, min_step=8):
        """ocrs_engine_edge_peaks: the directed edge peaks of pages of any sizes (a side at most 4096) at the angles of
        sc_table (int32 [A, 2]: skew_table) -> uint64 [n, 2 families, 2 signs, A, 16], in one launch."""
        n = len(inputs)
        t = np.ascontiguousarray(sc_table, np.int32).reshape(-1, 2)
        out = np.zeros((n, 2, 2, len(t), 16), np.uint64)
        check(lib().ocrs_engine_edge_peaks(self._h, _page_array(inputs), C.c_size_t(n), t.ctypes.data_as(C.POINTER(C.c_int32)),
                                           C.c_size_t(len(t)), C.c_int(int(min_step)), out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def find_outline(self, inp, **params):
        """ocrs_engine_find_outline -> Outline: the four corners of the sheet a photo shows (params: outline_params'
        keywords).  Uncalibrated on real photographs."""
        p, info = _outline_struct(**params), _lib.OutlineInfo()
        check(lib().ocrs_engine_find_outline(self._h, inp._h, C.byref(p), C.byref(info)))
        return _outline_of(info)

    def project(self, inp, m, out_hw, fill=0.5):
        """ocrs_engine_project_page: the page seen through the projective map m (eight coefficients: output pixel -> page
        position) as a new resident page of out_hw = (height, width); a tap outside the page is `fill`."""
        return self.project_batch([inp], [m], [out_hw], [fill])[0]

    def project_batch(self, inputs, ms, out_hws, fills=0.5):
        """ocrs_engine_project_pages: pages of any sizes, each with its own map, size and fill (or one fill for all), in
        one launch."""
        n = len(inputs)
        if not isinstance(fills, (list, tuple, np.ndarray)):
            fills = [fills] * n
        if len(ms) != n or len(out_hws) != n or len(fills) != n:
            raise ValueError("project_batch: one map, one size and one fill per page")
        mm = np.ascontiguousarray(np.concatenate([_map8_arg(m) for m in ms]) if n else np.zeros(0), np.float32)
        hw = (C.c_int * (2 * n))(*[int(v) for s in out_hws for v in (s[0], s[1])])
        fl = np.ascontiguousarray(np.asarray(fills, np.float32).reshape(-1))
        out = (C.c_void_p * n)()
        check(lib().ocrs_engine_project_pages(self._h, _page_array(inputs), C.c_size_t(n), hw, mm.ctypes.data_as(C.POINTER(C.c_float)),
                                              fl.ctypes.data_as(C.POINTER(C.c_float)), out))
        return _new_inputs(out, n)

    def straighten(self, inp, corners=None, fill=0.5):
        """The sheet a photo shows, upright -> (page, m, outline).  corners: TL, TR, BR, BL as (x, y) (None: what
        find_outline finds; outline is then its Outline, else None).  m is the map of the projection (quad_map):
        unproject_rects / unproject_lines with it bring results back to inp's frame.  When nothing is found inp itself
        comes back, with the identity map."""
        outline = None
        if corners is None:
            outline = self.find_outline(inp)
            if not outline.found:
                return inp, quad_map(page_corners(inp.shape[-2:]))[1], outline
            corners = outline.corners
        out_hw, m = quad_map(corners)
        return self.project(inp, m, out_hw, fill=fill), m, outline

    # ---- working resolution
    def resize(self, inp, size, filter="auto"):
        """ocrs_engine_resize_page: the page resampled to size = (height, width) as a new resident page.  filter: "area"
        (the exact area average; only shrinks), "bilinear" (the detection path's resize) or "auto" (area when neither side
        grows, else bilinear)."""
        return self.resize_batch([inp], [size], [filter])[0]

    def resize_batch(self, inputs, sizes, filters="auto"):
        """ocrs_engine_resize_pages: pages of any sizes, each to its own size with its own filter (or one for all), in one
        launch."""
        n = len(inputs)
        if isinstance(filters, str):
            filters = [filters] * n
        if len(sizes) != n or len(filters) != n:
            raise ValueError("resize_batch: one size and one filter per page")
        pages = _page_array(inputs)
        hw = (C.c_int * (2 * n))(*[int(v) for s in sizes for v in (s[0], s[1])])
        fl = (C.c_int * n)(*[_lib.RESAMPLE_FILTERS[f] for f in filters])
        out = (C.c_void_p * n)()
        check(lib().ocrs_engine_resize_pages(self._h, pages, C.c_size_t(n), hw, fl, out))
        return _new_inputs(out, n)

    # ---- lib.rs:193-199
    def detect_words(self, inp, scores=False, tiled=False, work_size=None, work_filter="auto", work_text_height=None):
        """scores=True: through ocrs_engine_detect_words_scored -> (words, score float32 [n], pixels uint32 [n]): per word
        the mean text probability of its component's pixels and their number.
        tiled=True | <overlap>: through ocrs_engine_detect_words_tiled: the page is cut into model-sized tiles at its own
        resolution instead of being resized to the model input (about one detector run per tile).
        work_size=(h, w): through ocrs_engine_detect_words_at: the detector sees the page resampled to that size (filter
        work_filter, as resize) and the words come back in the page's own frame; scores and pixels are those of the work
        page.  work_size() makes one from a scale or a longest side.
        work_text_height=N | True: the work size is the one at which the page's measured text is N pixels tall (True:
        WORK_TEXT_HEIGHT_DEFAULT), within a scale of 1/8 .. 4 (text_scale, work_scale_for_text, work_size); then as work_size.  Not
        together with work_size.  None launches nothing more than before."""
        if work_text_height is not None and work_text_height is not False:
            if work_size is not None:
                raise ValueError("detect_words: work_size or work_text_height, not both")
            work_size = self._work_size_for_text(inp, work_text_height)
        if work_size is not None:
            out = self.detect_words_batch([inp], scores, tiled, [work_size], work_filter)
            return tuple(o[0] for o in out) if scores else out[0]
        rects = C.POINTER(C.c_float)()
        n = C.c_size_t(0)
        overlap = _tile_overlap(tiled)
        if overlap is not None:
            sc, px = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
            check(lib().ocrs_engine_detect_words_tiled(self._h, inp._h, C.c_int(overlap), C.byref(rects), C.byref(n),
                                                       C.byref(sc) if scores else None, C.byref(px) if scores else None))
        elif scores:
            sc, px = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
            check(lib().ocrs_engine_detect_words_scored(self._h, inp._h, C.byref(rects), C.byref(n), C.byref(sc), C.byref(px)))
        else:
            check(lib().ocrs_engine_detect_words(self._h, inp._h, C.byref(rects), C.byref(n)))
        out = _take_rects(rects, n.value)
        if not scores:
            return out
        return out, _take(sc, n.value, np.float32), _take(px, n.value, np.uint32)

    def detect_words_batch(self, inputs, scores=False, tiled=False, work_sizes=None, work_filter="auto"):
        """scores=True: -> (words per page, score per page, pixels per page).  tiled: as detect_words.  work_sizes: one
        (h, w) or None (the page's own size) per page, as detect_words' work_size; resampled in one launch."""
        return _detect_words_batch("ocrs_engine_detect_words_batch", self._h, inputs, scores, tiled, work_sizes, work_filter)

    # ---- lib.rs:207-213
    def detect_text_pixels(self, inp, tiled=False):
        """tiled=True | <overlap>: the stitched map of the tiled call."""
        _, h, w = inp.shape
        out = np.empty((h, w), np.float32)
        overlap = _tile_overlap(tiled)
        if overlap is not None:
            check(lib().ocrs_engine_detect_text_pixels_tiled(self._h, inp._h, C.c_int(overlap), out.ctypes.data_as(C.POINTER(C.c_float))))
        else:
            check(lib().ocrs_engine_detect_text_pixels(self._h, inp._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    # ---- lib.rs:222-228
    def find_text_lines(self, inp, words, index=False):
        """index=True: -> (lines, index per line): index[l][k] is the position in `words` of rect k of line l."""
        a = _rects_to_array(words)
        lr = C.POINTER(C.c_float)()
        lo = C.POINTER(C.c_size_t)()
        nl = C.c_size_t(0)
        args = (self._h, inp._h if inp is not None else None, a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(len(a)),
                C.byref(lr), C.byref(lo), C.byref(nl))
        if index:
            wi = C.POINTER(C.c_size_t)()
            check(lib().ocrs_engine_find_text_lines_indexed(*args, C.byref(wi)))
        else:
            check(lib().ocrs_engine_find_text_lines(*args))
        offs = [lo[i] for i in range(nl.value + 1)]
        flat = _take_rects(lr, len(a))
        lib().ocrs_buffer_free(lo)
        lines = [flat[offs[i]:offs[i + 1]] for i in range(nl.value)]
        if not index:
            return lines
        widx = _take(wi, len(a), np.uintp).astype(np.int64)
        return lines, [widx[offs[i]:offs[i + 1]] for i in range(nl.value)]

    def find_text_lines_batch_raw(self, words_per_page, index=False):
        """Threaded over pages.  Returns (rects [n,6], line_offsets, page_line_offsets) as numpy arrays; index=True: plus
        word_index [n] (for every output rect its position in its page's input words)."""
        n = len(words_per_page)
        woffs = np.zeros(n + 1, dtype=np.uintp)
        for i, w in enumerate(words_per_page):
            woffs[i + 1] = woffs[i] + len(w)
        allw = np.ascontiguousarray(np.concatenate([_rects_to_array(w) for w in words_per_page]) if n else np.zeros((0, 6), np.float32))
        lr = C.POINTER(C.c_float)()
        lo = C.POINTER(C.c_size_t)()
        po = C.POINTER(C.c_size_t)()
        args = (self._h, C.c_size_t(n), allw.ctypes.data_as(C.POINTER(C.c_float)), woffs.ctypes.data_as(C.POINTER(C.c_size_t)),
                C.byref(lr), C.byref(lo), C.byref(po))
        if index:
            wi = C.POINTER(C.c_size_t)()
            check(lib().ocrs_engine_find_text_lines_batch_indexed(*args, C.byref(wi)))
        else:
            check(lib().ocrs_engine_find_text_lines_batch(*args))
        poffs = np.ctypeslib.as_array(po, shape=(n + 1,)).astype(np.uintp)
        nl = int(poffs[n])
        loffs = np.ctypeslib.as_array(lo, shape=(nl + 1,)).astype(np.uintp)
        rects = _take_rects(lr, len(allw))
        for p in (lo, po):
            lib().ocrs_buffer_free(p)
        if index:
            return rects, loffs, poffs, _take(wi, len(allw), np.uintp).astype(np.int64)
        return rects, loffs, poffs

    def recognize_text_batch_raw(self, inputs, rects, line_offsets, page_line_offsets, scores=False, rectify=False):
        """Packed form of recognize_text_batch: returns (chars, char_offsets) where chars is a
        structured array (ch, top, left, bottom, right) and line i owns chars[char_offsets[i]:char_offsets[i+1]].
        scores=True: returns (chars, char_offsets, char_logp float32 [len(chars)], line_score float64 [lines]), every
        line scored, those without text included.  rectify=True: rectified crops."""
        n = len(inputs)
        pages = _page_array(inputs)
        rects = np.ascontiguousarray(rects, np.float32)
        lo = np.ascontiguousarray(line_offsets, np.uintp)
        po = np.ascontiguousarray(page_line_offsets, np.uintp)
        nl = len(lo) - 1
        chars = C.POINTER(_lib.TextCharC)()
        coffs = C.POINTER(C.c_size_t)()
        args = [self._h, pages, C.c_size_t(n), po.ctypes.data_as(C.POINTER(C.c_size_t)),
                rects.ctypes.data_as(C.POINTER(C.c_float)), lo.ctypes.data_as(C.POINTER(C.c_size_t)), C.c_size_t(nl),
                C.byref(chars), C.byref(coffs)]
        if scores:
            clp, lsc = C.POINTER(C.c_float)(), C.POINTER(C.c_double)()
        if rectify:
            check(lib().ocrs_engine_recognize_text_batch_rectified(*args, C.byref(clp) if scores else None,
                                                                   C.byref(lsc) if scores else None))
        elif scores:
            check(lib().ocrs_engine_recognize_text_batch_scored(*args, C.byref(clp), C.byref(lsc)))
        else:
            check(lib().ocrs_engine_recognize_text_batch(*args))
        co = np.ctypeslib.as_array(coffs, shape=(nl + 1,)).astype(np.uintp)
        total = int(co[nl])
        dt = np.dtype([("ch", np.uint32), ("top", np.int32), ("left", np.int32), ("bottom", np.int32), ("right", np.int32)])
        if total:
            buf = (C.c_char * (total * dt.itemsize)).from_address(C.addressof(chars.contents))
            arr = np.frombuffer(buf, dtype=dt, count=total).copy()
        else:
            arr = np.zeros(0, dt)
        lib().ocrs_buffer_free(chars)
        lib().ocrs_buffer_free(coffs)
        if not scores:
            return arr, co
        char_logp = np.ctypeslib.as_array(clp, shape=(max(total, 1),))[:total].copy()
        line_score = np.ctypeslib.as_array(lsc, shape=(max(nl, 1),))[:nl].copy()
        lib().ocrs_buffer_free(clp)
        lib().ocrs_buffer_free(lsc)
        return arr, co, char_logp, line_score

    # ---- lib.rs:237-256
    def recognize_text(self, inp, lines, scores=False, rectify=False):
        """OcrEngine::recognize_text (lib.rs:237-256) through the single-page entry point a Rust binding uses.
        scores=True: through ocrs_engine_recognize_text_scored; every TextChar gets its logp, every TextLine its score.
        rectify=True: through ocrs_engine_recognize_text_rectified: every line is cropped along its own axis."""
        rects, offs = _pack_lines(lines)
        chars = C.POINTER(_lib.TextCharC)()
        coffs = C.POINTER(C.c_size_t)()
        args = [self._h, inp._h, rects.ctypes.data_as(C.POINTER(C.c_float)), offs.ctypes.data_as(C.POINTER(C.c_size_t)),
                C.c_size_t(len(lines)), C.byref(chars), C.byref(coffs)]
        clp = lsc = None
        if scores:
            clp, lsc = C.POINTER(C.c_float)(), C.POINTER(C.c_double)()
        if rectify:
            check(lib().ocrs_engine_recognize_text_rectified(*args, C.byref(clp) if scores else None, C.byref(lsc) if scores else None))
        elif scores:
            check(lib().ocrs_engine_recognize_text_scored(*args, C.byref(clp), C.byref(lsc)))
        else:
            check(lib().ocrs_engine_recognize_text(*args))
        out = [_line_from_c(chars, coffs, clp, lsc, li) for li in range(len(lines))]
        for p in (chars, coffs, clp, lsc):
            if p is not None:
                lib().ocrs_buffer_free(p)
        return out

    def recognize_text_batch(self, inputs, lines_per_page, scores=False, rectify=False):
        n = len(inputs)
        pages = _page_array(inputs)
        all_lines = [l for lines in lines_per_page for l in lines]
        plo = [0]
        for lines in lines_per_page:
            plo.append(plo[-1] + len(lines))
        rects, offs = _pack_lines(all_lines)
        plo_a = np.array(plo, dtype=np.uintp)
        chars = C.POINTER(_lib.TextCharC)()
        coffs = C.POINTER(C.c_size_t)()
        args = [self._h, pages, C.c_size_t(n), plo_a.ctypes.data_as(C.POINTER(C.c_size_t)),
                rects.ctypes.data_as(C.POINTER(C.c_float)), offs.ctypes.data_as(C.POINTER(C.c_size_t)),
                C.c_size_t(len(all_lines)), C.byref(chars), C.byref(coffs)]
        clp = lsc = None
        if scores:
            clp, lsc = C.POINTER(C.c_float)(), C.POINTER(C.c_double)()
        if rectify:
            check(lib().ocrs_engine_recognize_text_batch_rectified(*args, C.byref(clp) if scores else None,
                                                                   C.byref(lsc) if scores else None))
        elif scores:
            check(lib().ocrs_engine_recognize_text_batch_scored(*args, C.byref(clp), C.byref(lsc)))
        else:
            check(lib().ocrs_engine_recognize_text_batch(*args))
        result = []
        li = 0
        for lines in lines_per_page:
            page_out = []
            for _ in lines:
                page_out.append(_line_from_c(chars, coffs, clp, lsc, li))
                li += 1
            result.append(page_out)
        for p in (chars, coffs, clp, lsc):
            if p is not None:
                lib().ocrs_buffer_free(p)
        return result

    def recognize_tokens(self, inp, lines, rectify=False):
        """Raw greedy-CTC output per line: list of (label, pos) — CtcHypothesis::steps().  rectify=True: over rectified
        crops."""
        rects, offs = _pack_lines(lines)
        lab = C.POINTER(C.c_uint32)()
        pos = C.POINTER(C.c_uint32)()
        toff = C.POINTER(C.c_size_t)()
        fn = lib().ocrs_engine_recognize_tokens_rectified if rectify else lib().ocrs_engine_recognize_tokens
        check(fn(self._h, inp._h, rects.ctypes.data_as(C.POINTER(C.c_float)),
                 offs.ctypes.data_as(C.POINTER(C.c_size_t)), C.c_size_t(len(lines)), C.byref(lab), C.byref(pos), C.byref(toff)))
        out = []
        for i in range(len(lines)):
            out.append([(int(lab[k]), int(pos[k])) for k in range(toff[i], toff[i + 1])])
        for p in (lab, pos, toff):
            lib().ocrs_buffer_free(p)
        return out

    def recognize_logits(self, inp, lines):
        """The recognition model's log-probabilities per line, [T_i, classes] each (ocrs_engine_recognize_logits)."""
        rects, offs = _pack_lines(lines)
        lp = C.POINTER(C.c_float)()
        roff = C.POINTER(C.c_size_t)()
        ncls = C.c_int(0)
        check(lib().ocrs_engine_recognize_logits(self._h, inp._h, rects.ctypes.data_as(C.POINTER(C.c_float)),
                                                 offs.ctypes.data_as(C.POINTER(C.c_size_t)), C.c_size_t(len(lines)),
                                                 C.byref(lp), C.byref(roff), C.byref(ncls)))
        c = ncls.value
        out = []
        for i in range(len(lines)):
            a, b = roff[i], roff[i + 1]
            out.append(np.ctypeslib.as_array(lp, shape=(roff[len(lines)] * c,))[a * c:b * c].reshape(b - a, c).copy() if b > a
                       else np.zeros((0, c), np.float32))
        lib().ocrs_buffer_free(lp)
        lib().ocrs_buffer_free(roff)
        return out

    def run_recognition_ops(self, widths, first_op, last_op, inputs, gx_only=False):
        """Test hook (ocrs_engine_run_recognition_ops): recognition ops [first_op, last_op] through the engine's packed path
        over lines of model-input widths `widths`.  inputs: op first_op's input per line, the oracle's slot without its
        batch axis ([H, W, C] in the conv stack and at the TOSEQ, [T, 1, C] after it).  Returns op last_op's output per line
        in the same layout ([2, T, 3H] with gx_only)."""
        w = np.ascontiguousarray(widths, np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).ravel() for a in inputs]), np.float32)
        out = C.POINTER(C.c_float)()
        offs = C.POINTER(C.c_size_t)()
        shp = C.POINTER(C.c_int32)()
        check(lib().ocrs_engine_run_recognition_ops(self._h, w.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(len(w)),
                                                    int(first_op), int(last_op), int(bool(gx_only)),
                                                    flat.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(flat.size),
                                                    C.byref(out), C.byref(offs), C.byref(shp)))
        n = len(w)
        res = []
        for i in range(n):
            a, b = offs[i], offs[i + 1]
            d = (shp[3 * i], shp[3 * i + 1], shp[3 * i + 2])
            v = np.ctypeslib.as_array(out, shape=(max(offs[n], 1),))[a:b].copy() if b > a else np.zeros(0, np.float32)
            res.append(v.reshape(d))
        lib().ocrs_buffer_free(out)
        lib().ocrs_buffer_free(offs)
        lib().ocrs_buffer_free(shp)
        return res

    # ---- lib.rs:268-278
    def prepare_recognition_input(self, inp, line, rectify=False):
        """rectify=True: the rectified crop through ocrs_engine_prepare_recognition_input_rectified."""
        a = _rects_to_array(line)
        out = C.POINTER(C.c_float)()
        h, w = C.c_int(0), C.c_int(0)
        fn = lib().ocrs_engine_prepare_recognition_input_rectified if rectify else lib().ocrs_engine_prepare_recognition_input
        check(fn(self._h, inp._h, a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(len(a)), C.byref(out), C.byref(h), C.byref(w)))
        img = np.ctypeslib.as_array(out, shape=(max(h.value * w.value, 1),))[: h.value * w.value].reshape(h.value, w.value).copy()
        lib().ocrs_buffer_free(out)
        return img

    # ---- lib.rs:282-287
    def detection_threshold(self):
        return float(lib().ocrs_engine_detection_threshold(self._h))

    # ---- lib.rs:290-300
    def get_text(self, inp, rectify=False, orientation=None, work_size=None, normalize=None, deskew=None, deskew_fill=0.5,
                 perspective=None, perspective_fill=0.5, rules=None, despeckle=None, binarize=None, morph=None, frame=None, rank=None,
                 work_text_height=None, unreverse=None):
        """rectify=True: the same sequence (detect_words, find_text_lines, recognize_text) with rectified crops.
        orientation: None reads the page as given; an int turns it by that many quarter turns counter-clockwise first
        (rotate); "auto" by what detect_orientation finds.
        work_size=(h, w): the words are detected at that size of the (turned) page, lines and text are read from the page at
        its full resolution.
        normalize: None reads the page as given; True or a dict of normalize()'s keywords reads the normalised page
        (DESIGN.md §7.4).  Applied first; the turn, the work size and the crops are then those of the normalised page.
        deskew: None reads the page as given; a number straightens a skew of that many degrees first, "auto" one of what
        estimate_skew finds (deskew(); under 0.2 degrees the page is left alone).  Applied after
        normalisation, which puts paper at +0.5, the default deskew_fill, and after the turn.
        perspective: None reads the page as given; "auto" reads the sheet find_outline finds, four corners (TL, TR, BR, BL
        as (x, y)) the sheet they span (straighten()).  Applied first, before normalisation: the desk is cut
        away before normalisation looks at the paper.
        rules: None reads the page as given; True or a dict of remove_rules()'s keywords reads the page with its ruled lines
        removed.  Applied after perspective, normalisation, the turn and deskew, because rules must be
        axis-aligned, and before detection.
        despeckle: None reads the page as given; True or a dict of despeckle()'s keywords reads the page with its specks
        removed.  Applied after perspective and normalisation (it needs dark ink on light paper) and before
        the turn, deskew, whose interpolation would smear one-pixel specks into grey blobs, and rule removal.  Coordinates do
        not move.
        binarize: None reads the page as given; True or a dict of binarize()'s keywords reads the page cut into ink and
        paper by the local threshold.  Applied after perspective and normalisation (it needs dark ink on
        light paper) and before despeckling, the turn, deskew and rule removal, whose threshold 0 is then the local
        decision.  Coordinates do not move.
        morph: None reads the page as given; True or a dict of morph()'s keywords reads the page with its strokes repaired
        (DESIGN.md §7.11).  Applied last, before detection: after despeckling, so that specks are not grown or welded to
        text, and after rule removal, whose max_thickness a thickened rule would exceed.  Coordinates do not move.
        frame: None reads the page as given; True or a dict of frame()'s keywords reads the content box of the page with the
        ink connected to its frame removed.  Applied after perspective, normalisation and binarisation (it
        needs dark ink on light paper, and bars survive a binarisation) and before despeckling, the turn, deskew and rule
        removal, so that detect_orientation and estimate_skew no longer see the bars.  The crop moves coordinates; get_text
        returns text alone, so nothing is mapped back.
        rank: None reads the page as given; True or a dict of rank()'s keywords reads the page with its grain removed
        (DESIGN.md §7.13).  Applied after perspective and normalisation and before binarisation, which would turn grain into
        specks: everything downstream sees the cleaned page.  Coordinates do not move.
        work_text_height: None reads the page as given; N or True detects the words at the size at which the measured text
        is N pixels (True: WORK_TEXT_HEIGHT_DEFAULT) tall.  The page is measured as the detector will
        see it, after every operation above; lines and text are read at full resolution, as with work_size.  Not together
        with work_size.
        unreverse: None reads the page as given; True or a dict of unreverse()'s keywords reads the page with its
        reverse-video panels inverted.  Applied after perspective, normalisation, grain removal and
        binarisation and before frame, which would remove a sidebar that touches the edge as a bar; despeckling and
        everything later then see one polarity.  Coordinates do not move.
        get_text returns text alone; callers that want boxes run the steps
        themselves and bring them back last with unproject_rects / unproject_lines."""
        if perspective is not None:
            inp = self.straighten(inp, None if isinstance(perspective, str) and perspective == "auto" else perspective, fill=perspective_fill)[0]
        if normalize is not None and normalize is not False:
            inp = self.normalize(inp, **({} if normalize is True else dict(normalize)))
        if rank is not None and rank is not False:
            inp = self.rank(inp, **({} if rank is True else dict(rank)))
        if binarize is not None and binarize is not False:
            inp = self.binarize(inp, **({} if binarize is True else dict(binarize)))
        if unreverse is not None and unreverse is not False:
            inp = self.unreverse(inp, **({} if unreverse is True else dict(unreverse)))
        if frame is not None and frame is not False:
            inp = self.frame(inp, **({} if frame is True else dict(frame)))[0]
        if despeckle is not None and despeckle is not False:
            inp = self.despeckle(inp, **({} if despeckle is True else dict(despeckle)))
        if orientation is not None:
            k = self.detect_orientation(inp).quarter_turns if orientation == "auto" else int(orientation)
            inp = self.rotate(inp, k)
        if deskew is not None:
            inp = self.deskew(inp, None if deskew == "auto" else float(deskew), fill=deskew_fill)[0]
        if rules is not None and rules is not False:
            inp = self.remove_rules(inp, **({} if rules is True else dict(rules)))
        if morph is not None and morph is not False:
            inp = self.morph(inp, **({} if morph is True else dict(morph)))
        if work_text_height is False:
            work_text_height = None
        if work_size is not None and work_text_height is not None:
            raise ValueError("get_text: work_size or work_text_height, not both")
        if work_size is not None or work_text_height is not None or rectify:
            lines = self.find_text_lines(inp, self.detect_words(inp, work_size=work_size, work_text_height=work_text_height))
            return "\n".join(str(t) for t in self.recognize_text(inp, lines, rectify=rectify) if t is not None)
        txt = C.c_char_p()
        check(lib().ocrs_engine_get_text(self._h, inp._h, C.byref(txt)))
        s = txt.value.decode("utf-8")
        lib().ocrs_buffer_free(txt)
        return s

    # ---- measurement hooks
    def enable_timing(self, level=1):
        """0 off, 1 per-stage HIP-event timers, 2 also per-launch kernel-class timers."""
        check(lib().ocrs_engine_enable_timing(self._h, int(level)))

    def set_kernel_timing_classes(self, names=None):
        """Restrict per-launch kernel timing to the named classes (None = all)."""
        n = lib().ocrs_kernel_class_count()
        all_names = [lib().ocrs_kernel_class_name(i).decode() for i in range(n)]
        mask = 0xFFFFFFFF if names is None else sum(1 << all_names.index(x) for x in names)
        check(lib().ocrs_engine_set_kernel_timing_mask(self._h, C.c_uint32(mask)))

    def kernel_stats(self, reset=True):
        n = lib().ocrs_kernel_class_count()
        ms = (C.c_double * n)()
        cnt = (C.c_uint64 * n)()
        fl = (C.c_double * n)()
        by = (C.c_double * n)()
        mf = (C.c_double * n)()
        check(lib().ocrs_engine_kernel_mfma_flops(self._h, mf))
        check(lib().ocrs_engine_kernel_stats(self._h, ms, cnt, fl, by, 1 if reset else 0))
        return {lib().ocrs_kernel_class_name(i).decode(): dict(ms=ms[i], launches=int(cnt[i]), flops=fl[i], bytes=by[i],
                                                               mfma_flops=mf[i])
                for i in range(n)}

    def stage_times(self, reset=True):
        n = lib().ocrs_stage_count()
        ms = (C.c_double * n)()
        cnt = (C.c_uint64 * n)()
        check(lib().ocrs_engine_stage_times(self._h, ms, cnt, 1 if reset else 0))
        return {lib().ocrs_stage_name(i).decode(): (ms[i], int(cnt[i])) for i in range(n)}

    def __del__(self):
        try:
            if self._h and getattr(self, "_owned", True):
                lib().ocrs_engine_free(self._h)
            self._h = None
        except Exception:
            pass


def _line_from_c(chars, coffs, clp, lsc, li):
    """Line li of a recognize_text output as a TextLine (None: no text); clp / lsc: the scored call's arrays or None."""
    a, b = coffs[li], coffs[li + 1]
    if b <= a:
        return None
    return TextLine([TextChar(chr(chars[k].ch), (chars[k].top, chars[k].left, chars[k].bottom, chars[k].right),
                              None if clp is None else np.float32(clp[k])) for k in range(a, b)],
                    None if lsc is None else float(lsc[li]))


def _chars_from_c(chars, coffs, nl):
    co = np.ctypeslib.as_array(coffs, shape=(nl + 1,)).astype(np.uintp)
    total = int(co[nl])
    dt = np.dtype([("ch", np.uint32), ("top", np.int32), ("left", np.int32), ("bottom", np.int32), ("right", np.int32)])
    if total:
        buf = (C.c_char * (total * dt.itemsize)).from_address(C.addressof(chars.contents))
        arr = np.frombuffer(buf, dtype=dt, count=total).copy()
    else:
        arr = np.zeros(0, dt)
    lib().ocrs_buffer_free(chars)
    lib().ocrs_buffer_free(coffs)
    return arr, co


class EngineGroup:
    """Several GPUs behind one handle in one process (include/ocrs_amd.h "engine group"): a page is processed by a
    member of the device it lives on; pages the group places itself go out in contiguous blocks.  `devices` may repeat
    a device (members then share it; RCCL refuses such a communicator and the gathers use the host transport)."""

    GATHER = {"auto": 0, "host": 1, "rccl": 2}

    def __init__(self, devices, detection_bytes=None, recognition_bytes=None, debug=False, decode_method=DecodeMethod.Greedy,
                 alphabet=None, allowed_chars=None, gather="auto", numerics="exact", coalesce=0, coalesce_pages=0,
                 coalesce_window_us=0, layout_threads=0, rec_max_pixels=0, min_block=0, shared_block=0):
        p = _lib.GroupParams()
        p.numerics = NUMERICS[numerics]
        p.coalesce, p.coalesce_pages, p.coalesce_window_us = int(coalesce), int(coalesce_pages), int(coalesce_window_us)
        p.layout_threads, p.rec_max_pixels = int(layout_threads), int(rec_max_pixels)
        p.min_block, p.shared_block = int(min_block), int(shared_block)
        self._det = bytes(detection_bytes) if detection_bytes is not None else None
        self._rec = bytes(recognition_bytes) if recognition_bytes is not None else None
        p.detection_model = C.cast(C.c_char_p(self._det), C.c_void_p) if self._det else None
        p.detection_model_len = len(self._det) if self._det else 0
        p.recognition_model = C.cast(C.c_char_p(self._rec), C.c_void_p) if self._rec else None
        p.recognition_model_len = len(self._rec) if self._rec else 0
        self._devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        p.devices = self._devs
        p.n_devices = len(devices)
        p.debug = 1 if debug else 0
        p.decode_method = 0 if decode_method[0] == "greedy" else 1
        p.beam_width = decode_method[1]
        p.alphabet = alphabet.encode("utf-8") if alphabet is not None else None
        p.allowed_chars = allowed_chars.encode("utf-8") if allowed_chars is not None else None
        p.gather = self.GATHER[gather]
        self._h = C.c_void_p()
        check(lib().ocrs_engine_group_new(C.byref(p), C.byref(self._h)))
        self.devices = [int(d) for d in devices]

    def __len__(self):
        n = C.c_size_t(0)
        check(lib().ocrs_engine_group_size(self._h, C.byref(n)))
        return n.value

    def member(self, i):
        """(OcrEngine view of member i, its device)"""
        e, d = C.c_void_p(), C.c_int(-1)
        check(lib().ocrs_engine_group_member(self._h, C.c_size_t(i), C.byref(e), C.byref(d)))
        return OcrEngine._borrowed(e, self), d.value

    def member_stats(self, i):
        """ocrs_group_member_stats as a dict."""
        v = (C.c_uint64 * 8)()
        check(lib().ocrs_group_member_stats(self._h, C.c_size_t(i), v))
        return {"device": int(v[7]), "shares": int(v[0]), "pages": int(v[1]), "host_cpu_s": v[2] / 1e9, "busy_wall_s": v[3] / 1e9,
                "numa_node": int(v[4]) - 1 if v[4] else None, "node_cpus": int(v[5]), "bound_shares": int(v[6])}

    def set_option(self, name, value):
        """ocrs_engine_set_option on every member."""
        for i in range(len(self)):
            self.member(i)[0].set_option(name, value)

    def last_gather(self):
        t, b, why = C.c_int(0), C.c_size_t(0), C.c_char_p()
        check(lib().ocrs_group_last_gather(self._h, C.byref(t), C.byref(b), C.byref(why)))
        return {"transport": {0: None, 1: "host", 2: "rccl"}[t.value], "bytes": b.value,
                "why_host": (why.value or b"").decode()}

    def prepare_input_batch(self, images, order=DimOrder.Hwc):
        """images: equally shaped numpy arrays (host)."""
        arrs = [np.ascontiguousarray(a) for a in images]
        a0 = arrs[0]
        if order == DimOrder.Hwc:
            h, w, c = a0.shape
        else:
            c, h, w = a0.shape
        n = len(arrs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        out = (C.c_void_p * n)()
        check(lib().ocrs_group_prepare_input_batch(self._h, ptrs, C.c_size_t(n), 0 if a0.dtype == np.uint8 else 1, order, h, w, c, out))
        return _new_inputs(out, n)

    def prepare_input_device_batch(self, d_ptrs, dtype, order, h, w, c):
        n = len(d_ptrs)
        ptrs = (C.c_void_p * n)(*d_ptrs)
        out = (C.c_void_p * n)()
        check(lib().ocrs_group_prepare_input_device_batch(self._h, ptrs, C.c_size_t(n), 0 if dtype == np.uint8 else 1, order,
                                                          h, w, c, out))
        return _new_inputs(out, n)

    def detect_words_batch(self, inputs, scores=False, tiled=False):
        """scores=True: -> (words per page, score per page, pixels per page), as OcrEngine.detect_words_batch; tiled likewise."""
        return _detect_words_batch("ocrs_group_detect_words_batch", self._h, inputs, scores, tiled)

    def find_text_lines_batch_raw(self, words_per_page, index=False):
        return self.member(0)[0].find_text_lines_batch_raw(words_per_page, index=index)   # host work: any engine handle serves

    def recognize_text_batch_raw(self, inputs, rects, line_offsets, page_line_offsets, rectify=False):
        """rectify=True: through ocrs_group_recognize_text_batch_rectified."""
        n = len(inputs)
        pages = _page_array(inputs)
        rects = np.ascontiguousarray(rects, np.float32)
        lo = np.ascontiguousarray(line_offsets, np.uintp)
        po = np.ascontiguousarray(page_line_offsets, np.uintp)
        nl = len(lo) - 1
        chars = C.POINTER(_lib.TextCharC)()
        coffs = C.POINTER(C.c_size_t)()
        fn = lib().ocrs_group_recognize_text_batch_rectified if rectify else lib().ocrs_group_recognize_text_batch
        check(fn(
            self._h, pages, C.c_size_t(n), po.ctypes.data_as(C.POINTER(C.c_size_t)),
            rects.ctypes.data_as(C.POINTER(C.c_float)), lo.ctypes.data_as(C.POINTER(C.c_size_t)), C.c_size_t(nl),
            C.byref(chars), C.byref(coffs)))
        return _chars_from_c(chars, coffs, nl)

    def gather(self, payloads):
        """payloads: one bytes object per member -> (concatenation through the group's transport, offsets)."""
        g = len(self)
        assert len(payloads) == g
        bufs = [C.create_string_buffer(bytes(p), max(len(p), 1)) for p in payloads]
        ptrs = (C.c_void_p * g)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_size_t * g)(*[len(p) for p in payloads])
        out = C.c_void_p()
        offs = (C.c_size_t * (g + 1))()
        check(lib().ocrs_group_gather(self._h, ptrs, sizes, C.byref(out), offs))
        data = C.string_at(out, offs[g])
        lib().ocrs_buffer_free(out)
        return data, [int(offs[i]) for i in range(g + 1)]

    def final_gather(self, payloads, mode="auto"):
        """The end-of-stream result gather: like gather(), the transport named per call (auto = RCCL when it can be had)."""
        g = len(self)
        assert len(payloads) == g
        bufs = [C.create_string_buffer(bytes(p), max(len(p), 1)) for p in payloads]
        ptrs = (C.c_void_p * g)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_size_t * g)(*[len(p) for p in payloads])
        out = C.c_void_p()
        offs = (C.c_size_t * (g + 1))()
        check(lib().ocrs_group_final_gather(self._h, C.c_int(self.GATHER[mode]), ptrs, sizes, C.byref(out), offs))
        data = C.string_at(out, offs[g])
        lib().ocrs_buffer_free(out)
        return data, [int(offs[i]) for i in range(g + 1)]

    def set_replay(self, mode, seconds=(0.0, 0.0, 0.0)):
        """ocrs_group_set_replay (test hook): 0 off, 1 record per-page results, 2 replay them after sleeping seconds[stage]."""
        arr = (C.c_double * 3)(*[float(x) for x in seconds])
        check(lib().ocrs_group_set_replay(self._h, int(mode), arr))

    def worker_threads(self):
        n = C.c_size_t(0)
        check(lib().ocrs_group_worker_threads(self._h, C.byref(n)))
        return n.value

    def __del__(self):
        try:
            if self._h:
                lib().ocrs_engine_group_free(self._h)
                self._h = None
        except Exception:
            pass
