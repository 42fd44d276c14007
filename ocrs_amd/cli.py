"""`python -m ocrs_amd.cli image.png` — the call sequence of ocrs-cli
(ocrs-cli/src/main.rs:366-497) on the MI355X engine: load models, decode the
image to RGB u8 HWC (main.rs:312-323), prepare_input -> detect_words ->
find_text_lines -> recognize_text, print text or JSON.

Differences that are forced by the environment: models are `.ocrsm` files
(--detect-model / --rec-model; there is no network to download the default
`.rten` files from, main.rs:305-309) — with neither flag the seeded synthetic
models of ocrs_amd.models are used; the annotated-PNG output (-p) is not provided.
The debug dumps (--text-map / --text-mask / --text-line-images, main.rs:422-444)
write the same greyscale PNGs as the reference: (x.clamp(0,1) * 255) as u8
(main.rs:44-51).
"""
import os
import argparse
import sys

import numpy as np

from . import _lib


def load_image(path):
    """main.rs:312-323: image::open(..).into_rgb8() -> [H, W, 3] u8."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def write_image(path, chw_or_hw):
    """main.rs:21-51: float tensor in [0, 1] -> 8-bit greyscale PNG, `(x.clamp(0., 1.) * 255.0) as u8` (truncating)."""
    from PIL import Image
    a = np.asarray(chw_or_hw, np.float32)
    a = a.reshape(a.shape[-2], a.shape[-1])
    Image.fromarray((np.clip(a, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8), "L").save(path)


def positive_int(text):
    """argparse type of --work-text-height N."""
    n = int(text)
    if n <= 0:
        raise argparse.ArgumentTypeError("a positive number of pixels, not %r" % text)
    return n


def main(argv=None):
    ap = argparse.ArgumentParser(prog="ocrs_amd", description="Extract text from an image (MI355X engine).")
    ap.add_argument("image")
    ap.add_argument("--detect-model")
    ap.add_argument("--rec-model")
    ap.add_argument("--alphabet")
    ap.add_argument("--allowed-chars")
    ap.add_argument("--beam", action="store_true", help="beam search decoding (width 100, main.rs:403-404)")
    ap.add_argument("-j", "--json", action="store_true")
    ap.add_argument("--confidence", action="store_true",
                    help="with -j: a \"confidence\" per line and word, exp of the mean log-prob of its chars (no reference "
                         "counterpart; uncalibrated: DESIGN.md \"Recognition confidence\")")
    ap.add_argument("--detection-confidence", action="store_true",
                    help="with -j: \"word_boxes\" per line, the detector's word boxes in reading order with \"confidence\" (mean "
                         "text probability of the box's pixels) and \"pixels\" (no reference counterpart; uncalibrated: "
                         "DESIGN.md 7.1)")
    ap.add_argument("--min-word-score", type=float, metavar="X",
                    help="drop detected words whose detection confidence is below X before lines are formed")
    ap.add_argument("--tiled", nargs="?", type=int, const=-1, default=None, metavar="OVERLAP",
                    help="tiled detection for pages larger than the detector's input: the page is cut into model-sized tiles "
                         "at its own resolution, OVERLAP pixels shared between neighbours (default 100), instead of being "
                         "resized; about one detector run per tile (no reference counterpart: DESIGN.md 7.2)")
    ap.add_argument("--rectify", action="store_true",
                    help="crop every text line along its own axis instead of from its axis-aligned bounding box: for skewed "
                         "scans (no reference counterpart: DESIGN.md 8.4); also applies to --text-line-images")
    ap.add_argument("--orientation", choices=("0", "90", "180", "270", "auto"), default=None, metavar="{0,90,180,270,auto}",
                    help="turn the page counter-clockwise by that many degrees on the GPU before reading it, for scans that went "
                         "through the feeder sideways or upside down; auto: the turn the engine's probe finds (uncalibrated on "
                         "the synthetic models).  Boxes are reported in the frame of the file as given; the JSON gains "
                         "\"orientation\" (no reference counterpart: DESIGN.md 8.5)")
    work = ap.add_mutually_exclusive_group()
    work.add_argument("--work-scale", type=float, metavar="S",
                      help="detect words on the page resampled by S on the GPU (area average when shrinking, bilinear when "
                           "enlarging) and read the text from the page at its full resolution; boxes are reported in the frame of "
                           "the file (no reference counterpart; what a detector gains is uncalibrated on the synthetic models: "
                           "DESIGN.md 7.3)")
    work.add_argument("--work-max-side", type=int, metavar="N",
                      help="as --work-scale with S = min(1, N / the page's longer side): the detector sees a page of at most N "
                           "pixels a side")
    work.add_argument("--work-text-height", type=positive_int, nargs="?", const=True, default=None, metavar="N",
                      help="as --work-scale with the S at which the page's text is N pixels tall (default %d), within 1/8 to 4: the "
                           "text height is measured on the GPU from the page's connected components, without a detector, on the "
                           "page as the detector will see it; N is a positive number of pixels (write --work-text-height=N, or put another "
                           "option after the bare flag, so that the image path is not read as N); a blank page keeps its size; implies what --measure reports (no "
                           "reference counterpart; for real models the default is uncalibrated: DESIGN.md 7.14)" % _lib.WORK_TEXT_HEIGHT_DEFAULT)
    ap.add_argument("--measure", action="store_true",
                    help="measure the page's stroke width and text height on the GPU (run-length histograms and the bounding boxes of "
                         "connected components) and print them; with -j the JSON gains \"measure\" (no reference counterpart: "
                         "DESIGN.md 7.14)")
    ap.add_argument("--normalize", action="store_true",
                    help="normalise the page on the GPU before reading it: the background is flattened (shadows, uneven light), "
                         "the levels are stretched (faint copies) and light text on a dark page is inverted; the JSON gains "
                         "\"normalize\" (no reference counterpart; what a detector gains is uncalibrated: DESIGN.md 7.4)")
    ap.add_argument("--normalize-tile", type=int, default=None, metavar="N",
                    help="with --normalize: the tile the background is estimated over, a power of two from 16 to 256 (default 64)")
    ap.add_argument("--normalize-polarity", choices=("auto", "keep", "invert"), default=None,
                    help="with --normalize: auto (default) decides by a per-tile vote whether the page is light text on dark")
    ap.add_argument("--deskew", nargs="?", const="auto", default=None, metavar="auto|DEG",
                    help="straighten a page that went through the feeder a few degrees off, on the GPU, before reading it: DEG is "
                         "the skew in degrees, counter-clockwise, at most 45 either way; auto (the default) measures it from the "
                         "page's projection profiles, within 15 degrees (under 0.2 degrees the page is left alone).  Boxes are "
                         "reported in the frame of the file as given; the JSON gains \"skew\" (no reference counterpart: "
                         "DESIGN.md 7.6)")
    ap.add_argument("--deskew-fill", type=float, default=None, metavar="X",
                    help="with --deskew: the grey level around the straightened page, -0.5 black .. 0.5 white (default 0.5, the "
                         "paper of a page that went through --normalize)")
    ap.add_argument("--perspective", nargs="?", const="auto", default=None, metavar="auto|x0,y0,...,x3,y3",
                    help="straighten a sheet photographed at an angle, on the GPU, before anything else looks at it: eight numbers "
                         "are the sheet's corners in the file, top-left, top-right, bottom-right, bottom-left as x,y; auto (the "
                         "default) finds the sheet's outline against the desk (when none is found the page is read as given).  "
                         "Boxes are reported in the frame of the file as given; the JSON gains \"outline\" (no reference "
                         "counterpart; uncalibrated on real photographs: DESIGN.md 7.7)")
    ap.add_argument("--perspective-fill", type=float, default=None, metavar="X",
                    help="with --perspective: the grey level where the straightened sheet reaches beyond the photo, -0.5 black .. "
                         "0.5 white (default 0.5)")
    ap.add_argument("--remove-rules", action="store_true",
                    help="take the ruled lines of forms, tables and underlines out of the page on the GPU before reading it: long "
                         "thin runs of ink are overwritten with the paper's level, strokes that cross them are kept (after "
                         "--normalize, --orientation and --deskew: the rules must be axis-aligned dark ink on light paper); the "
                         "JSON gains \"rules\" (no reference counterpart; what a detector gains is uncalibrated: DESIGN.md 7.8)")
    ap.add_argument("--rules-min-length", type=int, default=None, metavar="N",
                    help="with --remove-rules: the shortest run of ink that is a rule, 2 to 65535 pixels (default 96)")
    ap.add_argument("--rules-max-thickness", type=int, default=None, metavar="N",
                    help="with --remove-rules: the thickest rule, 1 to 64 pixels (default 8); a thicker block is left alone")
    ap.add_argument("--rules-margin", type=int, default=None, metavar="N",
                    help="with --remove-rules: rows and columns of a rule's half-tone edge that go with it, 0 to 8 (default 1)")
    ap.add_argument("--despeckle", action="store_true",
                    help="take salt-and-pepper noise out of the page on the GPU before reading it: connected components of ink of "
                         "at most --speck-max-area pixels are overwritten with the paper's level (after --normalize, before "
                         "--orientation, --deskew and --remove-rules: it needs dark ink on light paper, and a warp smears specks); "
                         "the JSON gains \"despeckle\" (no reference counterpart; what a detector gains is uncalibrated: DESIGN.md 7.9)")
    ap.add_argument("--speck-max-area", type=int, default=None, metavar="N",
                    help="with --despeckle: the largest component of ink that is a speck, 0 to 4096 pixels (default 4)")
    ap.add_argument("--speck-fill-holes", type=int, default=None, metavar="N",
                    help="with --despeckle: also fill the light holes inside ink of at most N pixels, 0 to 4096, with the ink's level "
                         "(default 0: none; small values already close real counters of small glyphs)")
    ap.add_argument("--speck-keep-near", type=int, default=None, metavar="N",
                    help="with --despeckle: keep a speck that lies within N pixels of larger ink, 0 to 16 (default 0: keep none); for "
                         "i-dots and full stops when --speck-max-area is large")
    ap.add_argument("--unreverse", action="store_true",
                    help="turn reverse-video regions to dark on light on the GPU before reading the page: solid dark panels that "
                         "enclose light marks (a table's header band, the buttons and sidebars of a screenshot, a dark code pane) are "
                         "inverted with what they enclose (after --normalize and --binarize, before --frame, which would remove a "
                         "sidebar at the edge, and --despeckle); the JSON gains \"unreverse\" (no reference counterpart; the defaults "
                         "and what a detector gains are uncalibrated: DESIGN.md 7.15)")
    ap.add_argument("--unreverse-min-height", type=int, default=None, metavar="N",
                    help="with --unreverse: the least height of a panel's box, 1 to 65535 pixels (default 32, uncalibrated)")
    ap.add_argument("--unreverse-min-width", type=int, default=None, metavar="N",
                    help="with --unreverse: the least width of a panel's box, 1 to 65535 pixels (default 64, uncalibrated)")
    ap.add_argument("--unreverse-min-fill", type=float, default=None, metavar="X",
                    help="with --unreverse: the least share of its box a panel's ink fills, 0 to 1 (default 0.4, uncalibrated); a table "
                         "grid or a page frame fills less")
    ap.add_argument("--unreverse-min-holes", type=int, default=None, metavar="N",
                    help="with --unreverse: the enclosed light marks that make a dark region a panel (default 3, uncalibrated; it keeps "
                         "a bold O, B or 8 out; 0 inverts solid bars too)")
    ap.add_argument("--unreverse-max-hole", type=int, default=None, metavar="N",
                    help="with --unreverse: an enclosed light region of more than N pixels (a light card with dark text of its own) is "
                         "left as it is (default 0: no limit, uncalibrated)")
    ap.add_argument("--binarize", action="store_true",
                    help="cut the page into ink and paper on the GPU before reading it, by Sauvola's local threshold over a "
                         "window around every pixel instead of one cut for the page (after --normalize, before --despeckle, "
                         "--orientation, --deskew and --remove-rules: it needs dark ink on light paper); the JSON gains "
                         "\"binarize\" (no reference counterpart; what a detector gains is uncalibrated: DESIGN.md 7.10)")
    ap.add_argument("--binarize-radius", type=int, default=None, metavar="N",
                    help="with --binarize: the window reaches N pixels to every side, 1 to 127 (default 15)")
    ap.add_argument("--binarize-k", type=float, default=None, metavar="X",
                    help="with --binarize: Sauvola's k, 0 to 1, rounded to 1/256 (default 0.34; 0 is the plain local mean)")
    ap.add_argument("--binarize-keep-ink", action="store_true",
                    help="with --binarize: ink keeps its own grey levels and only the paper is whitened")
    ap.add_argument("--morph", default=None, metavar="OP[:RX[xRY]]",
                    help="repair the strokes on the GPU before reading the page, by running minima and maxima over a window that "
                         "reaches RX pixels to the left and right and RY up and down (0 to 63, not both 0; default 1; RY defaults to "
                         "RX).  OP: close bridges gaps and breaks in the ink, open removes hairs and separates fused characters, "
                         "thicken grows the ink, thin shrinks it; e.g. --morph close, --morph thicken:1x0 (applied last, after "
                         "--despeckle and --remove-rules; the JSON gains \"morph\"; no reference counterpart; what a detector gains "
                         "is uncalibrated: DESIGN.md 7.11)")
    ap.add_argument("--rank", nargs="?", const="", default=None, metavar="R[xRY]][:PERCENT[:TAIL]",
                    help="take grain (sensor noise, salt and pepper, a halftone screen) out of the page on the GPU before reading "
                         "it, by a rank filter over a window that reaches R pixels to the left and right and RY up and down (0 to "
                         "7, not both 0; default 1; RY defaults to R).  PERCENT: the rank taken, 0 to 100 (default 50, the median); "
                         "TAIL: 0 filters every pixel, 1 to 50 only the pixels whose rank in their window lies in the outer TAIL "
                         "percent (default 20: hairlines and small print are kept); e.g. --rank, --rank 2, --rank 1x0:50:0 (after "
                         "--normalize, before --binarize; the JSON gains \"rank\"; no reference counterpart; what a detector "
                         "gains is uncalibrated: DESIGN.md 7.13)")
    ap.add_argument("--frame", action="store_true",
                    help="take what surrounds the text out of the page on the GPU before reading it: ink that is connected to the "
                         "page's edges (scanner bars, the wedge of a skewed sheet, a slice of the neighbouring page) is overwritten "
                         "with the paper's level and the page is cut down to its content (after --normalize and --binarize, before "
                         "--despeckle, --orientation, --deskew and --remove-rules: it needs dark ink on light paper, and the probes "
                         "no longer see the bars).  Boxes are reported in the frame of the file as given; the JSON gains \"frame\" "
                         "(no reference counterpart; what a detector gains is uncalibrated: DESIGN.md 7.12)")
    ap.add_argument("--frame-depth", type=int, default=None, metavar="N",
                    help="with --frame or --split-spread: only ink within N pixels of the nearest edge is looked at, 0 to 65535 "
                         "(default 128; 0: the whole page)")
    ap.add_argument("--frame-sides", default=None, metavar="LTRB",
                    help="with --frame or --split-spread: the edges whose ink is removed, letters out of LTRB (default all four)")
    ap.add_argument("--frame-min-area", type=int, default=None, metavar="N",
                    help="with --frame or --split-spread: ink at an edge of fewer than N pixels is kept (default 0: none is)")
    ap.add_argument("--frame-pad", type=int, default=None, metavar="N",
                    help="with --frame or --split-spread: the margin kept around the content, 0 to 65535 pixels (default 16)")
    ap.add_argument("--crop", default=None, metavar="X0,Y0,X1,Y1",
                    help="read only that rectangle of the file (half open; it may reach beyond the file, where it is white), cut out "
                         "on the GPU before anything else looks at the page.  Boxes are reported in the frame of the file as given "
                         "(DESIGN.md 7.12)")
    ap.add_argument("--split-spread", action="store_true",
                    help="read the two pages of a book spread one after the other, the left page's text first: as --frame, and the "
                         "content is cut at the gutter, the widest column-run without ink near its middle (a page without one is "
                         "read whole)")
    ap.add_argument("-o", "--output")
    ap.add_argument("--debug", action="store_true")
    ap.add_argument("--text-map", action="store_true", help="write text-map.png (detect_text_pixels)")
    ap.add_argument("--text-mask", action="store_true", help="write text-mask.png (text map > detection threshold)")
    ap.add_argument("--numerics", choices=("exact", "relaxed", "reduced"), default="exact",
                    help="ocrs_engine_params.numerics (no reference counterpart): exact = bits of the CPU restatement (default); "
                         "relaxed / reduced = faster arithmetic whose outputs are expected, not guaranteed, to match (DESIGN.md 4.4)")
    ap.add_argument("--text-line-images", action="store_true",
                    help="write lines/line-N.png: the pre-processed recognition input of every text line")
    args = ap.parse_args(argv)
    if args.confidence and not args.json:
        ap.error("--confidence is only valid with -j/--json")
    if args.detection_confidence and not args.json:
        ap.error("--detection-confidence is only valid with -j/--json")
    if (args.normalize_tile is not None or args.normalize_polarity is not None) and not args.normalize:
        ap.error("--normalize-tile and --normalize-polarity are only valid with --normalize")
    if args.deskew_fill is not None and args.deskew is None:
        ap.error("--deskew-fill is only valid with --deskew")
    if (args.rules_min_length is not None or args.rules_max_thickness is not None or args.rules_margin is not None) and not args.remove_rules:
        ap.error("--rules-min-length, --rules-max-thickness and --rules-margin are only valid with --remove-rules")
    if (args.speck_max_area is not None or args.speck_fill_holes is not None or args.speck_keep_near is not None) and not args.despeckle:
        ap.error("--speck-max-area, --speck-fill-holes and --speck-keep-near are only valid with --despeckle")
    if (args.binarize_radius is not None or args.binarize_k is not None or args.binarize_keep_ink) and not args.binarize:
        ap.error("--binarize-radius, --binarize-k and --binarize-keep-ink are only valid with --binarize")
    unreverse_kw = {key: getattr(args, "unreverse_" + key) for key in ("min_height", "min_width", "min_fill", "min_holes", "max_hole")
                    if getattr(args, "unreverse_" + key) is not None}
    if unreverse_kw and not args.unreverse:
        ap.error("--unreverse-min-height, --unreverse-min-width, --unreverse-min-fill, --unreverse-min-holes and --unreverse-max-hole are "
                 "only valid with --unreverse")
    morph_kw = None
    if args.morph is not None:
        import re

        from . import MORPH_OPS
        m = re.fullmatch(r"([a-z]+)(?::(\d+)(?:x(\d+))?)?", args.morph)
        if not m or m.group(1) not in MORPH_OPS:
            ap.error("--morph: OP[:RX[xRY]] with OP one of %s, e.g. close, close:2, thicken:1x0; not %r" % (", ".join(MORPH_OPS), args.morph))
        rx = 1 if m.group(2) is None else int(m.group(2))
        morph_kw = {"op": m.group(1), "rx": rx, "ry": rx if m.group(3) is None else int(m.group(3))}
    rank_kw = None
    if args.rank is not None:
        import re
        m = re.fullmatch(r"(?:(\d+)(?:x(\d+))?)?(?::(\d+)(?::(\d+))?)?", args.rank)
        if not m:
            ap.error("--rank: [R[xRY]][:PERCENT[:TAIL]], e.g. 1, 2x1, 1:50, 1x0:50:0; not %r" % args.rank)
        rx = 1 if m.group(1) is None else int(m.group(1))
        rank_kw = {"rx": rx, "ry": rx if m.group(2) is None else int(m.group(2)), "percent": 50 if m.group(3) is None else int(m.group(3)),
                   "tail": 20 if m.group(4) is None else int(m.group(4))}
    frame_kw = {}
    if (args.frame_depth is not None or args.frame_sides is not None or args.frame_min_area is not None or args.frame_pad is not None) \
            and not (args.frame or args.split_spread):
        ap.error("--frame-depth, --frame-sides, --frame-min-area and --frame-pad are only valid with --frame or --split-spread")
    if args.frame_sides is not None:
        if not args.frame_sides or any(c not in "LTRB" for c in args.frame_sides.upper()):
            ap.error("--frame-sides: letters out of LTRB, not %r" % args.frame_sides)
        frame_kw["sides"] = args.frame_sides
    for name, key in (("frame_depth", "depth"), ("frame_min_area", "min_area"), ("frame_pad", "pad")):
        if getattr(args, name) is not None:
            frame_kw[key] = getattr(args, name)
    crop_rect = None
    if args.crop is not None:
        try:
            crop_rect = tuple(int(v) for v in args.crop.split(","))
        except ValueError:
            crop_rect = ()
        if len(crop_rect) != 4 or not all(abs(v) < 2 ** 31 for v in crop_rect):
            ap.error("--crop takes four integers X0,Y0,X1,Y1")
    if args.perspective_fill is not None and args.perspective is None:
        ap.error("--perspective-fill is only valid with --perspective")
    if args.perspective is not None and args.perspective != "auto":
        try:
            args.perspective = [float(v) for v in args.perspective.split(",")]
        except ValueError:
            ap.error("--perspective takes auto or eight numbers x0,y0,...,x3,y3")
        if len(args.perspective) != 8 or not all(np.isfinite(args.perspective)):
            ap.error("--perspective takes auto or eight numbers x0,y0,...,x3,y3")
    if args.deskew is not None and args.deskew != "auto":
        try:
            args.deskew = float(args.deskew)
        except ValueError:
            ap.error("--deskew takes auto or a number of degrees")
        if not abs(args.deskew) <= 45.0:
            ap.error("--deskew: at most 45 degrees either way (--orientation turns by quarter turns)")

    from . import DecodeMethod, DimOrder, ImageSource, Model, OcrEngine, models, output
    from ._lib import OcrsError
    det = Model.load_file(args.detect_model) if args.detect_model else Model.load_bytes(models.synthetic_detection_bytes())
    rec = Model.load_file(args.rec_model) if args.rec_model else Model.load_bytes(models.synthetic_recognition_bytes())
    engine = OcrEngine(detection_model=det, recognition_model=rec, debug=args.debug, alphabet=args.alphabet,
                       allowed_chars=args.allowed_chars, numerics=args.numerics,
                       decode_method=DecodeMethod.BeamSearch(100) if args.beam else DecodeMethod.Greedy)
    # JPEG files: Huffman decoding here, everything per-sample on the GPU (include/ocrs_amd.h "JPEG hand-off"); flavours
    # the hand-off does not cover, and every other format, are decoded on the host as the reference does (main.rs:312-323)
    inp, shape_hw = None, None
    with open(args.image, "rb") as f:
        head = f.read(2)
        if head == b"\xff\xd8" and not os.environ.get("OCRS_CLI_HOST_DECODE"):
            data = head + f.read()
            try:
                inp, coef_bytes = engine.prepare_input_jpeg(data)
                shape_hw = inp.shape[-2:]
                if args.debug:
                    print("JPEG hand-off: %d bytes of coefficients to the GPU for %dx%d pixels" % (coef_bytes, shape_hw[1], shape_hw[0]))
            except OcrsError as e:
                if e.status != 6:   # OCRS_ERR_IMAGE_SOURCE = a flavour to decode on the host
                    raise
    if inp is None:
        img = load_image(args.image)
        shape_hw = img.shape[:2]
        inp = engine.prepare_input(ImageSource.from_tensor(img, DimOrder.Hwc))
    if crop_rect is not None:   # from here on the zone is the page; results are mapped back last
        try:
            inp = engine.crop(inp, crop_rect, 0.5)   # white around a zone that reaches beyond the file
        except OcrsError as e:
            if e.status != 1:   # OCRS_ERR_INVALID_ARGUMENT: a side outside 1 .. 65535
                raise
            ap.error("--crop: %s" % e)
    outline, quad_m = None, None
    if args.perspective is not None:   # from here on the straightened sheet is the page; results are mapped back last
        corners = None if args.perspective == "auto" else np.array(args.perspective, np.float32).reshape(4, 2)
        try:
            flat, m, found = engine.straighten(inp, corners, fill=0.5 if args.perspective_fill is None else args.perspective_fill)
        except OcrsError as e:
            if e.status != 1 or corners is None:   # OCRS_ERR_INVALID_ARGUMENT: corners that span no area
                raise
            ap.error("--perspective: %s" % e)
        if found is not None and args.debug:
            print("Outline: %s, corners %s, polarity %d, edge pixels %s (taken at %dx%d)"
                  % ("found" if found.found else "none", found.corners.tolist(), found.polarity, list(found.counts), found.work_hw[1], found.work_hw[0]))
        outline = {"found": flat is not inp, "corners": (corners if found is None else found.corners).tolist()}
        if flat is not inp:
            inp, quad_m = flat, m
    norm_info = None
    if args.normalize:   # from here on the normalised page is the page; coordinates do not move
        inp, norm_info = engine.normalize(inp, tile=64 if args.normalize_tile is None else args.normalize_tile,
                                          polarity=args.normalize_polarity or "auto", info=True)
        if args.debug:
            print("Normalize: %s page (vote %d), white bin %d, levels %d .. %d, %d pixels counted"
                  % ("dark" if norm_info["dark"] else "light", norm_info["vote"], norm_info["white"], norm_info["lo"], norm_info["hi"],
                     norm_info["counted"]))
    rank_info = None
    if rank_kw is not None:   # from here on the page without its grain is the page; coordinates do not move
        try:
            inp, rank_info = engine.rank(inp, info=True, **rank_kw)
        except OcrsError as e:
            if e.status != 1:   # OCRS_ERR_INVALID_ARGUMENT: a parameter out of range
                raise
            ap.error("--rank: %s" % e)
        rank_info = dict(rank_info, **rank_kw)
        if args.debug:
            print("Rank: percent %d over %d x %d, tail %d: %d of %d counted pixels changed, %d spared; %d pixels of ink before, %d after"
                  % (rank_kw["percent"], 2 * rank_kw["rx"] + 1, 2 * rank_kw["ry"] + 1, rank_kw["tail"], rank_info["changed"],
                     rank_info["counted"], rank_info["spared"], rank_info["ink_before"], rank_info["ink_after"]))
    binarize_info = None
    if args.binarize:   # from here on the page cut into ink and paper is the page; coordinates do not move
        try:
            inp, binarize_info = engine.binarize(inp, radius=15 if args.binarize_radius is None else args.binarize_radius,
                                                 k=0.34 if args.binarize_k is None else args.binarize_k,
                                                 keep_ink=args.binarize_keep_ink, info=True)
        except (OcrsError, ValueError) as e:
            if isinstance(e, OcrsError) and e.status != 1:   # OCRS_ERR_INVALID_ARGUMENT: a parameter out of range
                raise
            ap.error("--binarize: %s" % e)
        if args.debug:
            print("Binarize: %d of %d counted pixels are ink, written as %g (kept: %s); paper written as %g"
                  % (binarize_info["ink"], binarize_info["counted"], binarize_info["ink_fill"],
                     "yes" if args.binarize_keep_ink else "no", binarize_info["paper_fill"]))
    unreverse_info = None
    if args.unreverse:   # from here on the page of one polarity is the page; coordinates do not move
        try:
            inp, unreverse_info = engine.unreverse(inp, info=True, **unreverse_kw)
        except OcrsError as e:
            if e.status != 1:   # OCRS_ERR_INVALID_ARGUMENT: a parameter out of range
                raise
            ap.error("--unreverse: %s" % e)
        if args.debug:
            print("Unreverse: %d panels (%d pixels) of %d candidates among %d components of ink inverted with %d holes (%d pixels), "
                  "%d holes over the limit left alone; %d pixels inverted, %d pixels of ink"
                  % (unreverse_info["panels"], unreverse_info["panel_pixels"], unreverse_info["candidates"], unreverse_info["components"],
                     unreverse_info["holes"], unreverse_info["hole_pixels"], unreverse_info["skipped_holes"], unreverse_info["inverted"],
                     unreverse_info["ink"]))
    def read_part(inp):
        """One page from despeckling to recognition, its results back in the frame `inp` has here."""
        turn_hw = inp.shape[-2:]   # the frame the turn's results come back to
        speckle_info = None
        if args.despeckle:   # from here on the page without its specks is the page; coordinates do not move
            try:
                inp, speckle_info = engine.despeckle(inp, max_area=4 if args.speck_max_area is None else args.speck_max_area,
                                                     max_hole=0 if args.speck_fill_holes is None else args.speck_fill_holes,
                                                     keep_near=0 if args.speck_keep_near is None else args.speck_keep_near, info=True)
            except OcrsError as e:
                if e.status != 1:   # OCRS_ERR_INVALID_ARGUMENT: a parameter out of range
                    raise
                ap.error("--despeckle: %s" % e)
            if args.debug:
                print("Despeckle: %d specks (%d pixels) overwritten with %g (paper bin %d of %d pixels counted), %d kept near larger ink "
                      "(%d pixels), %d holes (%d pixels) filled with %g (ink bin %d); %d pixels of ink"
                      % (speckle_info["specks"], speckle_info["speck_pixels"], speckle_info["paper_fill"], speckle_info["paper_bin"],
                         speckle_info["counted"], speckle_info["kept"], speckle_info["kept_pixels"], speckle_info["holes"],
                         speckle_info["hole_pixels"], speckle_info["ink_fill"], speckle_info["ink_bin"], speckle_info["ink"]))
        turns = None
        if args.orientation is not None:   # from here on the turned page is the page; results are mapped back before output
            if args.orientation == "auto":
                found = engine.detect_orientation(inp)
                turns = found.quarter_turns
                if args.debug:
                    print("Orientation: vote %s (horizontal : vertical), scores %s over %s chars -> %d degrees"
                          % (found.vote.tolist(), found.scores.tolist(), found.n_chars.tolist(), 90 * turns))
            else:
                turns = int(args.orientation) // 90
            inp = engine.rotate(inp, turns)
        skew, skew_map = None, None
        if args.deskew is not None:   # from here on the upright page is the page; results are mapped back before output
            skew = args.deskew
            if skew == "auto":
                found = engine.estimate_skew(inp)
                skew = found.angle
                if args.debug:
                    print("Skew: %.1f degrees (scores: best coarse %d, runner-up %d, at the angle %d; taken at %dx%d)"
                          % (skew, found.scores[0], found.scores[1], found.scores[2], found.work_hw[1], found.work_hw[0]))
            upright, m, _ = engine.deskew(inp, skew, fill=0.5 if args.deskew_fill is None else args.deskew_fill)
            if upright is inp:
                skew = 0.0
            else:
                inp, skew_map = upright, m
        rules_info = None
        if args.remove_rules:   # from here on the page without its rules is the page; coordinates do not move
            try:
                inp, rules_info = engine.remove_rules(inp, min_length=96 if args.rules_min_length is None else args.rules_min_length,
                                                      max_thickness=8 if args.rules_max_thickness is None else args.rules_max_thickness,
                                                      margin=1 if args.rules_margin is None else args.rules_margin, info=True)
            except OcrsError as e:
                if e.status != 1:   # OCRS_ERR_INVALID_ARGUMENT: a parameter out of range
                    raise
                ap.error("--remove-rules: %s" % e)
            if args.debug:
                print("Rules: %d pixels overwritten with %g (paper bin %d of %d pixels counted): %d of horizontal rules, %d of vertical "
                      "rules, %d kept where a stroke crosses; %d pixels of ink"
                      % (rules_info["overwritten"], rules_info["fill"], rules_info["paper_bin"], rules_info["counted"],
                         rules_info["h_removed"], rules_info["v_removed"], rules_info["kept"], rules_info["ink"]))
        morph_info = None
        if morph_kw is not None:   # from here on the page with its strokes repaired is the page; coordinates do not move
            try:
                inp, morph_info = engine.morph(inp, info=True, **morph_kw)
            except OcrsError as e:
                if e.status != 1:   # OCRS_ERR_INVALID_ARGUMENT: a parameter out of range
                    raise
                ap.error("--morph: %s" % e)
            morph_info = dict(morph_info, **morph_kw)
            if args.debug:
                print("Morph: %s over %d x %d: %d of %d counted pixels changed; %d pixels of ink before, %d after"
                      % (morph_kw["op"], 2 * morph_kw["rx"] + 1, 2 * morph_kw["ry"] + 1, morph_info["changed"], morph_info["counted"],
                         morph_info["ink_before"], morph_info["ink_after"]))
        tiled = False if args.tiled is None else True if args.tiled < 0 else args.tiled
        work_hw = None   # the size the detector sees the (turned) page at: DESIGN.md 7.3
        if args.work_scale is not None or args.work_max_side is not None:
            from . import work_size
            work_hw = work_size(inp.shape[-2:], scale=args.work_scale, max_side=args.work_max_side)
        measure_info = None
        if args.measure or args.work_text_height is not None:   # of the page as the detector will see it
            from . import measure_choose, work_scale_for_text, work_size
            record = engine.measure(inp)
            scale = measure_choose(record)
            measure_info = dict(scale._asdict(), ink=record["ink"], components=record["components"])
            if args.work_text_height is not None:
                work_hw = work_size(inp.shape[-2:], scale=work_scale_for_text(scale.text_height, None if args.work_text_height is True else args.work_text_height))
            if args.debug or not args.json:
                print("Measure: %s; %d pixels of ink in %d components"
                      % ("a blank page: no text to measure" if scale.blank else
                         "strokes of %d pixels, text %d pixels tall (over %d components)" % (scale.stroke, scale.text_height, scale.support),
                         record["ink"], record["components"]))
        if work_hw is not None and args.debug:
            print("Working resolution: %dx%d for a page of %dx%d" % (work_hw[1], work_hw[0], inp.shape[-1], inp.shape[-2]))
        if args.text_map or args.text_mask:   # with a working resolution: the map of the work page, at its size
            tm = engine.detect_text_pixels(inp if work_hw is None else engine.resize(inp, work_hw), tiled=tiled)
            if args.text_map:
                write_image("text-map.png", tm)
            if args.text_mask:
                write_image("text-mask.png", (tm > np.float32(engine.detection_threshold())).astype(np.float32))
        word_boxes = None
        if args.detection_confidence or args.min_word_score is not None:
            words, wscore, wpixels = engine.detect_words(inp, scores=True, tiled=tiled, work_size=work_hw)
            if args.min_word_score is not None:
                keep = wscore >= np.float32(args.min_word_score)
                words, wscore, wpixels = words[keep], wscore[keep], wpixels[keep]
            lines, index = engine.find_text_lines(inp, words, index=True)
            if args.detection_confidence:
                word_boxes = [[(words[k], wscore[k], wpixels[k]) for k in idx] for idx in index]
        else:
            words = engine.detect_words(inp, tiled=tiled, work_size=work_hw)
            lines = engine.find_text_lines(inp, words)
        if args.text_line_images:  # main.rs:66-86
            os.makedirs("lines", exist_ok=True)
            for i, line in enumerate(lines):
                write_image("lines/line-%d.png" % i, engine.prepare_recognition_input(inp, line, rectify=args.rectify) + np.float32(0.5))
        texts = engine.recognize_text(inp, lines, scores=args.confidence, rectify=args.rectify)
        if skew_map is not None:
            from . import unwarp_lines, unwarp_rects
            texts = unwarp_lines(texts, skew_map)
            if word_boxes is not None:
                word_boxes = [[(unwarp_rects([r], skew_map)[0], s, n) for r, s, n in boxes] for boxes in word_boxes]
        if turns is not None:
            from . import unrotate_lines, unrotate_rects
            texts = unrotate_lines(texts, tuple(turn_hw), turns)
            if word_boxes is not None:
                word_boxes = [[(unrotate_rects([r], tuple(turn_hw), turns)[0], s, n) for r, s, n in boxes] for boxes in word_boxes]
        return {"texts": texts, "word_boxes": word_boxes, "words": words, "lines": lines, "turns": turns, "skew": skew,
                "despeckle": speckle_info, "rules": rules_info, "morph": morph_info, "measure": measure_info}

    # the pages to read and where each lies on the page as it is here: the content box, the two pages of a spread, or the page
    parts, frame_info = [(inp, None)], None
    if args.frame or args.split_spread:   # from here on what surrounds the text is gone
        try:
            if args.split_spread:
                parts, frame_info = engine.split_spread(inp, info=True, **frame_kw)
            else:
                page, origin, frame_info = engine.frame(inp, info=True, **frame_kw)
                parts = [(page, origin)]
        except (OcrsError, ValueError) as e:
            if isinstance(e, OcrsError) and e.status != 1:   # OCRS_ERR_INVALID_ARGUMENT: a parameter out of range
                raise
            ap.error("--frame: %s" % e)
        choice = frame_info.pop("choice")
        frame_info["boxes"] = [[o[0], o[1], o[0] + p.shape[-1], o[1] + p.shape[-2]] for p, o in parts]
        if args.debug:
            print("Frame: %d components (%d pixels) touching the frame overwritten with %g (paper bin %d of %d pixels counted), %d kept "
                  "(%d pixels); %d of %d pixels of ink in the ring; content %s, gutter at %d -> %s"
                  % (frame_info["removed"], frame_info["removed_pixels"], frame_info["paper_fill"], frame_info["paper_bin"],
                     frame_info["counted"], frame_info["kept"], frame_info["kept_pixels"], frame_info["ring_ink"], frame_info["ink"],
                     "found" if choice["found"] else "not found", choice["gutter_x"], frame_info["boxes"]))
    texts, word_boxes, words, lines = [], None, [], []
    for n_part, (part, origin) in enumerate(parts):   # the left page first
        got = read_part(part)
        if origin is not None:
            from . import uncrop_lines, uncrop_rects
            got["texts"] = uncrop_lines(got["texts"], origin)
            if got["word_boxes"] is not None:
                got["word_boxes"] = [[(uncrop_rects([r], origin)[0], s, n) for r, s, n in boxes] for boxes in got["word_boxes"]]
        texts += got["texts"]
        if got["word_boxes"] is not None:
            word_boxes = (word_boxes or []) + got["word_boxes"]
        words, lines = list(words) + list(got["words"]), list(lines) + list(got["lines"])
        if n_part == 0:   # what the later steps report is what they found on the first page
            turns, skew, speckle_info, rules_info, morph_info = got["turns"], got["skew"], got["despeckle"], got["rules"], got["morph"]
            measure_info = got["measure"]
    if quad_m is not None:
        from . import unproject_lines, unproject_rects
        texts = unproject_lines(texts, quad_m)
        if word_boxes is not None:
            word_boxes = [[(unproject_rects([r], quad_m)[0], s, n) for r, s, n in boxes] for boxes in word_boxes]
    if crop_rect is not None:
        from . import uncrop_lines, uncrop_rects
        texts = uncrop_lines(texts, crop_rect[:2])
        if word_boxes is not None:
            word_boxes = [[(uncrop_rects([r], crop_rect[:2])[0], s, n) for r, s, n in boxes] for boxes in word_boxes]
    if args.json:
        content = output.format_json_output(args.image, tuple(shape_hw), texts, confidence=args.confidence, word_boxes=word_boxes,
                                            orientation=None if turns is None else 90 * turns, normalize=norm_info, skew=skew, outline=outline,
                                            rules=rules_info, despeckle=speckle_info, binarize=binarize_info, morph=morph_info, frame=frame_info,
                                            rank=rank_info, measure=measure_info, unreverse=unreverse_info)
    else:
        content = output.format_text_output(texts)
    if args.output:
        with open(args.output, "w", encoding="utf-8") as f:
            f.write(content)
    else:
        print(content)
    if args.debug:
        print("Found %d words, %d lines in image of size %dx%d" % (len(words), len(lines), shape_hw[1], shape_hw[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
