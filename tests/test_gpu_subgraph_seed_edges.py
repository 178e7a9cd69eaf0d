"""kq_subgraph_seed_dev with a caller's device pointer at every offset of its 16-byte window, on the texts of
tests/scan_inputs.py (run ends and runs of exactly k bases at and across the tile and lane edges of the scanner), exact against
`seed` of tests/subgraph_ref.py on the same bytes.  The device copy of a text lies where tests/test_gpu_scan_edges.py puts it:
an aligned tensor + 64 + lead, bases in front and behind.  The database is counted from edge_table_reads (about half of the
text's k-mers with substitutions, a high-copy repeat), so both sources of a seed entry occur all over the text.

k = 21 and 32 also: the host entry (which stages the text at an aligned address) must export the same bytes; and a k-mer the
database lacks whose first occurrence starts in the last lane of a tile and whose second, with other neighbours, starts in the
first lane of the next tile of the same segment (tests/subgraph_inputs.py: tile_repeat_text) carries the edges of the first."""
import pytest

from tests import helpers as H
from tests import scan_inputs as S
from tests import subgraph_inputs as G
from tests import subgraph_ref as R
from tests.test_gpu_scan_edges import dev_text

pytestmark = pytest.mark.gpu

MAP = S.MAP
IDS = [f"k{k}-lead{lead}" for k, lead in S.CASES]
HOST_TOO = (21, 32)
REPEAT_CASES = [(k, lead) for k in (21, 32) for lead in S.LEADS]


@pytest.fixture(scope="module")
def kq():
    from kreeq_amd import capi
    assert capi.device_available()
    return capi


def new_sub(kq, k):
    return kq.KreeqDB(k, MAP, 0, capacity_hint=1 << 12)


@pytest.mark.parametrize("k,lead", S.CASES, ids=IDS)
def test_seed_dev(kq, k, lead):
    ref = S.reference(k, lead)
    table = R.table_of(ref.table)                                        # the oracle's table, once for both flag values
    db = kq.KreeqDB(k, MAP)
    db.count_batch(ref.reads)
    assert H.entries_equal(db.export(), ref.table)
    t, ptr = dev_text(ref.text, lead)
    assert ptr % 16 == lead
    for no_reference in (False, True):
        want = R.seed(table, [ref.text], k, no_reference)
        assert any(key in table for key in want) and (no_reference or any(key not in table for key in want))
        sub = new_sub(kq, k)
        db.subgraph_seed_dev(sub, ptr, len(ref.text), no_reference)
        got = sub.export()
        assert H.entries_equal(got, R.entries_of(want)), no_reference
        assert sub.summary() == R.summary(want, k)
        if k in HOST_TOO:
            host = new_sub(kq, k)
            db.subgraph_seed(host, ref.text, no_reference)
            assert host.export().tobytes() == got.tobytes(), no_reference
            host.close()
        sub.close()
    db.close()


@pytest.mark.parametrize("k,lead", REPEAT_CASES, ids=[f"k{k}-lead{lead}" for k, lead in REPEAT_CASES])
def test_first_occurrence_across_a_tile_edge(kq, k, lead):
    text, plants = G.tile_repeat_text(k, lead)
    db = kq.KreeqDB(k, MAP)
    db.count_batch(text[:2000])                                          # part of the text: database entries next to constructed ones
    table = R.table_of(db.export())
    want = R.seed(table, [text], k)
    for w, a, b, at in plants:
        key, f, bw = G.constructed(a, w, text[at + k:at + k + 1])
        assert key not in table and want[key] == (f, bw, 1)
        assert G.constructed(text[at + G.PERIOD - 1:at + G.PERIOD], w, b)[1:] != (f, bw)
    t, ptr = dev_text(text, lead)
    sub = new_sub(kq, k)
    db.subgraph_seed_dev(sub, ptr, len(text))
    got = sub.export()
    assert H.entries_equal(got, R.entries_of(want))
    for w, a, b, at in plants:                                           # said once more on the device's own answer
        key, f, bw = G.constructed(a, w, text[at + k:at + k + 1])
        e = sub.lookup_keys([key])[0]
        assert (e["fw"].tolist(), e["bw"].tolist(), int(e["cov"])) == (f, bw, 1)
    host = new_sub(kq, k)
    db.subgraph_seed(host, text)
    assert host.export().tobytes() == got.tobytes()
    for h in (sub, host, db):
        h.close()
