"""Output formats of ocrs-cli (ocrs-cli/src/output.rs): plain text and the
HierText-like JSON (`paragraphs[].lines[].{text, vertices, words[]}`)."""
import json
import math

from . import rotated_rect_corners


def _rround(v):  # f32::round — half away from zero
    return int(math.copysign(math.floor(abs(float(v)) + 0.5), float(v)))


def rounded_vertex_coords(rect6):
    """output.rs:24-27."""
    return [[_rround(x), _rround(y)] for x, y in rotated_rect_corners(rect6)]


def ocr_json(input_path, input_hw, text_lines, confidence=False, word_boxes=None, orientation=None, normalize=None, skew=None, outline=None, rules=None, despeckle=None, binarize=None, morph=None, frame=None, rank=None, measure=None, unreverse=None):
    """output.rs:34-76.  text_lines: list of TextLine | None.  confidence (no reference counterpart): every line and word
    object also gets "confidence" (TextLine / TextWord.confidence; the lines must come from a scored recognize_text).
    word_boxes (no reference counterpart; indexed like text_lines): per line the detector's word boxes in reading order as
    (rect6, score, pixels); every line object then gets "word_boxes": [{"vertices", "confidence", "pixels"}].
    orientation (no reference counterpart): the degrees the page was turned counter-clockwise before it was read; the top
    level then gets "orientation" (the boxes given here are already in the frame of the file).
    normalize (no reference counterpart): what OcrEngine.normalize(info=True) found on the page; the top level then gets
    "normalize": {"counted", "dark", "hi", "lo", "vote", "white"}.
    skew (no reference counterpart): the degrees of skew the page was straightened by before it was read (0 when it was
    left alone); the top level then gets "skew" (the boxes given here are already in the frame of the file).
    outline (no reference counterpart): {"found", "corners"} of the sheet the page was straightened to before it was read
    (corners: TL, TR, BR, BL as [x, y] in the frame of the file; found false: the page was read as given); the top level then
    gets "outline".
    rules (no reference counterpart): what OcrEngine.remove_rules(info=True) found on the page; the top level then gets
    "rules": {"counted", "fill", "h_removed", "ink", "kept", "overwritten", "paper_bin", "v_removed"}.
    despeckle (no reference counterpart): what OcrEngine.despeckle(info=True) found on the page; the top level then gets
    "despeckle": {"counted", "hole_pixels", "holes", "ink", "ink_bin", "ink_fill", "kept", "kept_pixels", "paper_bin",
    "paper_fill", "speck_pixels", "specks"}.
    binarize (no reference counterpart): what OcrEngine.binarize(info=True) counted on the page; the top level then gets
    "binarize": {"counted", "ink", "ink_fill", "paper_fill"}.
    morph (no reference counterpart): what OcrEngine.morph(info=True) counted on the page, with the op and the radii it was
    asked for; the top level then gets "morph": {"changed", "counted", "ink_after", "ink_before", "op", "rx", "ry"}.
    frame (no reference counterpart): what OcrEngine.clean_frame(info=True) found on the page, with "boxes": the rectangles
    [x0, y0, x1, y1] that were read, in reading order (one, or the two pages of a spread); the top level then gets "frame":
    {"boxes", "counted", "ink", "kept", "kept_pixels", "paper_bin", "paper_fill", "removed", "removed_pixels", "ring_ink"}.
    rank (no reference counterpart): what OcrEngine.rank(info=True) counted on the page, with the radii, the percent and the
    tail it was asked for; the top level then gets "rank": {"changed", "counted", "ink_after", "ink_before", "percent", "rx",
    "ry", "spared", "tail"}.
    measure (no reference counterpart): the scale measure_choose made of OcrEngine.measure's record of the page the detector
    saw, with the record's ink and components; the top level then gets "measure": {"blank", "components", "ink", "stroke",
    "support", "text_height"}; blank (a bool) says that no text was found to measure.
    unreverse (no reference counterpart): what OcrEngine.unreverse(info=True) found on the page; the top level then gets
    "unreverse": {"candidates", "components", "hole_pixels", "holes", "ink", "inverted", "panel_pixels", "panels",
    "skipped_holes"}."""
    line_items = []
    for li, line in enumerate(text_lines):
        if line is None:
            continue
        words = []
        for w in line.words():
            words.append({"text": str(w), "vertices": rounded_vertex_coords(w.rotated_rect())})
            if confidence:
                words[-1]["confidence"] = w.confidence
        line_items.append({"text": str(line), "words": words, "vertices": rounded_vertex_coords(line.rotated_rect())})
        if confidence:
            line_items[-1]["confidence"] = line.confidence
        if word_boxes is not None:
            line_items[-1]["word_boxes"] = [{"vertices": rounded_vertex_coords(r), "confidence": float(s), "pixels": int(n)}
                                            for r, s, n in word_boxes[li]]
    height, width = input_hw
    doc = {"url": input_path, "image_width": width, "image_height": height, "paragraphs": [{"lines": line_items}]}
    if orientation is not None:
        doc["orientation"] = int(orientation)
    if normalize is not None:
        doc["normalize"] = {k: int(normalize[k]) for k in ("counted", "dark", "hi", "lo", "vote", "white")}
    if skew is not None:
        doc["skew"] = float(skew)
    if outline is not None:
        doc["outline"] = {"found": bool(outline["found"]), "corners": [[float(x), float(y)] for x, y in outline["corners"]]}
    if rules is not None:
        doc["rules"] = {k: int(rules[k]) for k in ("counted", "h_removed", "ink", "kept", "overwritten", "paper_bin", "v_removed")}
        doc["rules"]["fill"] = float(rules["fill"])
    if despeckle is not None:
        doc["despeckle"] = {k: (float if k.endswith("_fill") else int)(v) for k, v in despeckle.items()}
    if binarize is not None:
        doc["binarize"] = {k: (float if k.endswith("_fill") else int)(v) for k, v in binarize.items()}
    if morph is not None:
        doc["morph"] = {k: (str if k == "op" else int)(v) for k, v in morph.items()}
    if frame is not None:
        doc["frame"] = {k: (float if k.endswith("_fill") else int)(v) for k, v in frame.items() if k != "boxes"}
        doc["frame"]["boxes"] = [[int(v) for v in b] for b in frame["boxes"]]
    if rank is not None:
        doc["rank"] = {k: int(v) for k, v in rank.items()}
    if measure is not None:
        doc["measure"] = {k: int(measure[k]) for k in ("components", "ink", "stroke", "support", "text_height")}
        doc["measure"]["blank"] = bool(measure["blank"])
    if unreverse is not None:
        doc["unreverse"] = {k: int(v) for k, v in unreverse.items()}
    return doc


def format_json_output(input_path, input_hw, text_lines, confidence=False, word_boxes=None, orientation=None, normalize=None, skew=None, outline=None, rules=None, despeckle=None, binarize=None, morph=None, frame=None, rank=None, measure=None, unreverse=None):
    """output.rs:98-101 (serde_json::to_string_pretty).  serde_json without `preserve_order` keeps `json!` maps in a
    BTreeMap, so the reference emits every object's keys in alphabetical order (ocrs-cli/test-data/
    format-json-expected.json: image_height, image_width, paragraphs, url / text, vertices, words): sort_keys."""
    return json.dumps(ocr_json(input_path, input_hw, text_lines, confidence, word_boxes, orientation, normalize, skew, outline, rules, despeckle, binarize, morph, frame, rank, measure, unreverse), indent=2, ensure_ascii=False,
                      sort_keys=True)


def format_text_output(text_lines):
    """output.rs:88-95."""
    return "\n".join(str(l) for l in text_lines if l is not None)
