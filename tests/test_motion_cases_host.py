"""Host proofs that every case of tests/_motion_cases.py is what tests/test_gpu_motion_branches.py takes it for, on the
restatement (tests/_motion_ref.py) alone -- no GPU.  A case whose scene stopped discriminating (medians that agree, minima that
do not tie, a threshold that is not met with equality) fails here, not silently on the device."""
import numpy as np
import pytest

import _motion_cases as cases
import _motion_ref as ref


def _valid(g, rows):
    return [b for b, r in enumerate(rows) if ref.block_valid(r, g)]


def _true_shifts(c, shift):
    for s, shifts in enumerate(c['shifts']):
        assert shift[s, 0].tolist() == [0, 0, 0, 0]
        assert shift[s, 1:, :3].tolist() == [[dx, dy, 1] for dx, dy in shifts], (shift[s].tolist(), shifts)


def test_the_coarse_texture_is_what_k8_needs():
    """197 x 459, k = 8, R = 4, true shift (13, -29): ref.texture leaves a block's SAD range below the default min_texture and
    no motion is reported; the coarse texture recovers it."""
    hw, shifts = (197, 459), [(13, -29)]
    g = ref.Geometry(hw, 8, 4)
    off = ref.offsets_of_shifts(shifts, cases.MARGIN)
    for tex, ok in ((ref.texture(600, 800, 7), False), (cases.coarse(0), True)):
        st = ref.Stream(g)
        lumas = ref.crops(tex, hw, off).astype(np.int64)
        st.step(lumas[0])
        shift, blocks = st.step(lumas[1])
        assert (min(int(r[3] - r[2]) for r in blocks) >= 1024) == ok
        assert shift[:3].tolist() == ([13, -29, 1] if ok else [0, 0, 0])


@pytest.mark.parametrize('name', sorted(cases.INSTANCES))
def test_every_instance_case(name):
    """The geometry the table claims (k, neither side a multiple of k, odd sides, wr % 4 != 0, at least two blocks), shifts that
    are no multiple of k and reach +-R k, all of them recovered; the 16-bit layouts hold 1022 and 1023."""
    c = cases.INSTANCES[name]
    g, shift, _, _ = cases.want('instance', name)
    H, W = c['hw']
    assert g.k == c['k'] and H % g.k and W % g.k and H % 2 and W % 2 and g.wr % 4 and g.nb >= 2
    assert len(c['shifts']) == (2 if name in cases.TWO_STREAMS else 1)
    for shifts in c['shifts']:
        assert all(dx % g.k or dy % g.k for dx, dy in shifts) and any(g.R * g.k in (abs(dx), abs(dy)) for dx, dy in shifts)
    _true_shifts(c, shift)
    px, lumas = cases.scene('instance', name)
    if c['source'] in ('p010', 'i010'):
        v10 = ref.live_bits(px, c['source'])
        assert (v10 == 1022).any() and (v10 == 1023).any() and (v10 % 4 != 0).any() and (lumas == 255).any()
        assert np.array_equal(ref.luma_y(px, c['source']), np.minimum(255, (v10 + 2) >> 2))
        assert (np.asarray(px).view(np.uint16) != (v10 << 6 if c['source'] == 'p010' else v10)).any()         # ignored bits are set


def test_every_instance_has_a_case():
    names = set(cases.INSTANCES)
    for k in (4, 8):
        for source in ('rgb',) + cases.LAYOUTS:
            assert {f'{source}-k{k}-wide', f'{source}-k{k}-narrow'} <= names
    assert {f'{source}-k2-wide' for source in cases.LAYOUTS} <= names
    two = [cases.INSTANCES[n] for n in cases.TWO_STREAMS]
    assert {c['k'] for c in two} == {4, 8} and all(c['source'] != 'rgb' for c in two)


@pytest.mark.parametrize('name', sorted(cases.MEDIANS))
def test_medians_decide(name):
    """An even number of valid blocks below nb; lower and upper median differ in x and in y, coarse and final; the blocks that
    hold the x median are not those that hold the y median; the invalid blocks are the flat ones."""
    g, shift, blocks, _ = cases.want('medians', name)
    rows = blocks[0, 1]
    valid = _valid(g, rows)
    assert g.nb == 6 and valid == [0, 1, 3, 4] and shift[0, 1, 2:].tolist() == [1, 4]
    assert all(rows[b, 2] == rows[b, 3] == 0 for b in (2, 5))        # flat against flat
    for fx in (0, 4):
        (xl, xu), (yl, yu) = ref.medians(rows[valid, fx]), ref.medians(rows[valid, fx + 1])
        assert xl != xu and yl != yu, (name, fx, rows.tolist())
        assert not {b for b in valid if rows[b, fx] == xl} & {b for b in valid if rows[b, fx + 1] == yl}
    c = cases.MEDIANS[name]
    assert shift[0, 1, :2].tolist() == [min(c['a'][0], c['b'][0]), min(c['a'][1], c['b'][1])]
    assert sorted(rows[valid, 4:].tolist()) == sorted([list(c['a'])] * 2 + [list(c['b'])] * 2)


@pytest.mark.parametrize('name', sorted(cases.MANY))
def test_many_blocks_cases(name):
    """nb as stated, above the 256 threads of block_median; both motions are found, so the histograms have several bins."""
    c = cases.MANY[name]
    g, shift, blocks, _ = cases.want('many', name)
    assert g.nb == c['nb'] > 256 and shift[0, 1, 2] == 1 and shift[0, 1, 3] > 256
    rows = blocks[0, 1]
    valid = _valid(g, rows)
    assert len({int(v) for v in rows[valid, 0]}) > 1 and len({int(v) for v in rows[valid, 1]}) > 1
    found = {tuple(r) for r in rows[valid, 4:].tolist()}
    assert {c['a'], c['b']} <= found


@pytest.mark.parametrize('name', sorted(cases.PERIODIC))
def test_minima_tie(name):
    """The coarse SADs of a valid block: x / y -- several candidates share the minimum at the smallest distance, so dx (dy)
    decides; diagonal -- the smallest (dy, dx) among them is not the smallest (dx, dy), so the order of the two decides; both --
    candidates share it at unequal distances too, so the distance decides first."""
    c = cases.PERIODIC[name]
    g, shift, blocks, _ = cases.want('periodic', name)
    _, lumas = cases.scene('periodic', name)
    rows = blocks[0, 1]
    assert _valid(g, rows) == list(range(g.nb)) and shift[0, 1, 2] == 1
    sads = ref.coarse_sads(ref.reduce_luma(lumas[0, 0], g), ref.reduce_luma(lumas[0, 1], g), g, 0)
    least = min(sads.values())
    at = sorted((dy * dy + dx * dx, dy, dx) for (dy, dx), s in sads.items() if s == least)
    nearest = [t for t in at if t[0] == at[0][0]]
    assert least == rows[0, 2] and len(nearest) >= 2 and rows[0, :2].tolist() == [nearest[0][2], nearest[0][1]]
    if name == 'x':
        assert len({t[1] for t in nearest}) == 1 and len({t[2] for t in nearest}) > 1          # dx decides
    if name == 'y':
        assert len({t[1] for t in nearest}) > 1                                                # dy decides
    if name == 'diagonal':                                                                     # dy before dx decides
        by_dx = min((dx, dy) for _, dy, dx in nearest)
        assert [(dx, dy) for _, dy, dx in nearest] == [(2, -2), (-2, 2)] and (nearest[0][2], nearest[0][1]) != by_dx
    if name == 'both':
        assert len(at) > len(nearest)
        assert min((dy, dx) for _, dy, dx in at) != (nearest[0][1], nearest[0][2])             # without the distance: another one


@pytest.mark.parametrize('name', sorted(cases.ODD))
def test_odd_search_cases(name):
    c = cases.ODD[name]
    g, shift, _, _ = cases.want('odd', name)
    assert g.R % 2 and (16 + 2 * g.R) % 4 and g.nb >= 2
    assert any(g.R * g.k in (abs(dx), abs(dy)) for dx, dy in c['shifts'][0])
    _true_shifts(c, shift)


def test_thresholds_flip_at_equality():
    """min_texture at the least SAD range of a valid block keeps it, one more drops it; min_blocks at n_valid reports, one more
    does not."""
    g0, shift0, blocks0, _ = cases.want('medians', cases.THRESHOLD_BASE)
    n = int(shift0[0, 1, 3])
    got = {w: cases.want('threshold', w) for w in cases.THRESHOLDS}
    least = got['texture_equal'][0].min_texture
    assert least > g0.min_texture and got['texture_above'][0].min_texture == least + 1
    assert least == min(int(r[3] - r[2]) for r in blocks0[0, 1] if ref.block_valid(r, g0))
    assert got['texture_equal'][1][0, 1].tolist() == shift0[0, 1].tolist()
    assert got['texture_above'][1][0, 1, 3] < n and got['texture_above'][1][0, 1, 2] == 1
    assert (got['blocks_equal'][0].min_blocks, got['blocks_above'][0].min_blocks) == (n, n + 1)
    assert got['blocks_equal'][1][0, 1].tolist() == shift0[0, 1].tolist()
    assert got['blocks_above'][1][0, 1].tolist() == [0, 0, 0, n]
    assert not got['blocks_above'][2][0, 1, :, 4:].any() and np.array_equal(got['blocks_above'][2][0, 1, :, :4], blocks0[0, 1, :, :4])
