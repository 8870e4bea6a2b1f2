"""The table of asynchronous classes and plan layouts (tests/async_table.py) against the header and the host planner.
Runs without a GPU: an entry point added to include/muahuff.h fails here until it is classified, the "Conventions"
comment of the header must name exactly the entry points the table calls capturable, and a layout that no longer lands
in the planner form it names fails before any GPU run."""
import os
import re
import subprocess

from tests import async_table as at
from tests import helpers
from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "muahuff.h")


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(mh_[a-z_0-9]+)\s*\(", hdr))


def test_every_declared_entry_point_has_exactly_one_class():
    declared = _declared()
    assert declared == set(at.CLASS), dict(unclassified=sorted(declared - set(at.CLASS)),
                                           not_declared=sorted(set(at.CLASS) - declared))
    assert set(at.CLASS.values()) == {at.HOST, at.CAPTURABLE, at.SYNCHRONISES}
    # what the header documents to synchronise or allocate
    assert set(at.of_class(at.SYNCHRONISES)) == {
        "mh_decode_status", "mh_decode_range", "mh_decode_rebin", "mh_plan_create", "mh_plan_create_packed",
        "mh_plan_destroy", "mh_sweep_create", "mh_sweep_destroy"}
    # everything that takes a stream enqueues on it: capturable or synchronises, never host
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    with_stream = set(re.findall(r"\b(mh_[a-z_0-9]+)\s*\([^;]*?void \*stream\)", hdr))
    assert with_stream == set(at.of_class(at.CAPTURABLE)) | {"mh_decode_status", "mh_decode_range", "mh_decode_rebin"}


def test_header_conventions_name_the_capturable_set():
    text = open(HEADER).read()
    conv = text[text.index("Conventions"):text.index("#ifndef MUAHUFF_H")]
    conv = re.sub(r"\s*\n\s*\*\s*", " ", conv)               # one line, comment stars removed
    m = re.search(r"nothing in ([^;]*?) synchronises, allocates or frees, so they can be captured into a hipGraph", conv)
    assert m, "the Conventions comment no longer states the capture promise in its known wording"
    named = set(re.findall(r"mh_[a-z_0-9]+", m.group(1)))
    want = set(at.of_class(at.CAPTURABLE))
    assert named == want, dict(header_only=sorted(named - want), table_only=sorted(want - named))
    # the per-function comments of the calls that are NOT capturable say so
    for name in ("mh_decode_range", "mh_decode_rebin"):
        body = text[text.rindex("/*", 0, text.index("int %s(" % name)):text.index("int %s(" % name)]
        assert re.search(r"(?i)not\s+capturable", body), name
    body = text[text.rindex("/*", 0, text.index("int mh_decode_status(")):text.index("int mh_decode_status(")]
    assert "Synchronises" in body


def test_layouts_use_both_decoder_families_and_every_form():
    assert [l.name for l in at.LAYOUTS] == ["a", "b", "c", "d"]
    assert any(l.S <= 4 for l in at.LAYOUTS) and any(l.S >= 7 for l in at.LAYOUTS)
    assert {(l.wave, l.S <= 4) for l in at.LAYOUTS} == {(True, True), (True, False), (False, True), (False, False)}
    a, b, c, d = at.LAYOUTS
    assert a.wave and a.measure_fused and a.fused_cal and a.tickets_fit and (1 << a.h) <= at.K_CAL_DIRECT
    assert not b.wave and not b.measure_fused and len(b.lens) > at.K_FUSED_MEASURE_CHANNELS
    assert c.wave and not c.fused_cal and c.cal_tiled and (1 << c.h) > at.K_CAL_DIRECT
    assert d.heads >= 1 and d.short >= 1 and d.skipped >= 2 and d.window == 0


def test_every_layout_lands_in_the_form_it_names(exe):  # noqa: F811
    tabs = helpers.sclv_tables()
    lines = []
    for l in at.LAYOUTS:
        rows = tabs[l.S]
        lines.append("%d %d %d %d %d %d %d 8  %s  %s" % (len(l.lens), l.S, l.h, l.mode, l.window, len(rows), l.seg_chunks,
                                                        " ".join(map(str, l.lens)),
                                                        " ".join(str(int(v)) for v in rows.ravel())))
    r = subprocess.run([exe, "--forms"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(at.LAYOUTS), r.stdout
    for g, l in zip(got, at.LAYOUTS):
        wave, fused, fcal, tickets, cal_tiles, heads, skipped, short = (int(v) for v in g.split())
        assert (bool(wave), bool(fused), bool(fcal), bool(tickets), cal_tiles > 0, heads, skipped, short) == \
               (l.wave, l.measure_fused, l.fused_cal, l.tickets_fit, l.cal_tiled, l.heads, l.skipped, l.short), (l.name, g)
