"""The poisoned arena (tests/arena.py) tests itself on the CPU with plain torch: a correct implementation of a shared-MLP layer on
arena-carved operands passes clean, and each planted mistake of the kinds the GPU cases exist for is reported by operand name."""
import pytest
import torch

from tests.arena import ACC_GUARD, Arena, GUARD_BYTES, ROW_TILE, poison_bits

R, CIN, LDX, LDW, COUT, LDY = 5, 6, 8, 12, 3, 4


def layer_arena():
    """Y (R,LDY)[:, :COUT] = X (R,LDX)[:, :CIN] . W (COUT,LDW)[:, :CIN]^T, stat (2*COUT + 1 float64) += [column sums of y | of y^2 | 0],
    arg (R,COUT) uint8 = 1 where y > 0, through a scratch of R*COUT doubles; idx is an integer input nobody should touch."""
    g = torch.Generator().manual_seed(5)
    a = Arena('cpu')
    a.inp('X', torch.randn(R, CIN, generator=g), ld=LDX)
    a.inp('W', torch.randn(COUT, CIN, generator=g), ld=LDW)
    a.inp('idx', torch.arange(R, dtype=torch.int64), fill=0)
    a.out('Y', (R, COUT), ld=LDY)
    a.out('arg', (R, COUT), dtype=torch.uint8)
    a.acc('stat', torch.arange(2 * COUT + 1, dtype=torch.float64) + 100.0)
    a.scratch('partial', R * COUT)
    return a.build()


def correct_layer(t):
    x, w = t['X'], t['W']
    y = x[:, :CIN] @ w[:, :CIN].t()
    t['partial'].copy_(y.double().reshape(-1))  # scratch: anything inside
    t['Y'][:, :COUT] = y
    t['arg'][:, :COUT] = (y > 0).to(torch.uint8)
    part = t['partial'].reshape(R, COUT)
    t['stat'][:COUT] += part.sum(0)
    t['stat'][COUT:2 * COUT] += (part * part).sum(0)


def test_layout_is_the_one_promised():
    a = layer_arena()
    for name, ld in (('X', LDX), ('W', LDW), ('Y', LDY)):
        t = a[name]
        assert t.stride() == (ld, 1) and t.data_ptr() % 16 == 0
        assert a.ops[name].guard * 4 >= max(GUARD_BYTES, ROW_TILE * ld * 4)
    assert a['stat'].data_ptr() % 16 == 8 and a['partial'].data_ptr() % 16 == 8  # the odd double offset of arena[2*C+1:]
    assert a['arg'].data_ptr() % 16 == 0 and a['idx'].data_ptr() % 16 == 0
    # pads and guards of a float operand: the quiet NaN with the payload; of the integer input: its valid fill; outputs: NaN / 0xA5 inside
    xf = a.flat[torch.float32].view(torch.int32)
    o = a.offset('X')
    assert int(xf[o - 1]) == poison_bits(torch.float32) and int(xf[o + CIN]) == poison_bits(torch.float32)
    assert torch.isnan(a.flat[torch.float32][o + CIN]) and torch.isnan(a['Y']).all() and torch.isnan(a['partial']).all()
    ii = a.flat[torch.int64]
    assert int(ii[a.offset('idx') - 1]) == 0 and int(ii[a.offset('idx') + R]) == 0
    assert int(a['arg'][0, 0]) == 0xA5
    assert a.check(nan_ok=('Y',)) == []  # nothing ran: nothing changed (Y is still unwritten, which nan_ok silences)


def test_packed_operands_are_back_to_back():
    a = Arena('cpu')
    a.acc('stat1', torch.full((7,), 11.0, dtype=torch.float64))
    a.acc('stat2', torch.full((9,), 22.0, dtype=torch.float64), pack=True)
    a.acc('zsum', torch.full((4,), 33.0, dtype=torch.float64), pack=True)
    a.build()
    assert a.offset('stat2') == a.offset('stat1') + 7 and a.offset('zsum') == a.offset('stat2') + 9
    assert a['stat1'].data_ptr() % 16 == 8 and a['stat2'].data_ptr() % 16 == 0
    a['stat2'].add_(1.0)
    assert a.check() == []
    a.flat[torch.float64][a.offset('stat2') + 9] = 5.0  # slot "2C+1" of stat2 is zsum[0] -- zsum may change, so this is legal ...
    assert a.check() == []
    a2 = Arena('cpu')
    a2.acc('stat1', torch.full((7,), 11.0, dtype=torch.float64))
    a2.inp('zsum', torch.full((4,), 33.0, dtype=torch.float64), pack=True)
    a2.build()
    a2.flat[torch.float64][a2.offset('stat1') + 7] = 5.0  # ... and a finding where the neighbour is not this call's to write
    assert any(f.startswith('zsum: input changed at element offset 0') for f in a2.check())


def test_the_reference_passes_clean_on_arena_and_on_clean_operands():
    a = layer_arena()
    correct_layer(a)
    assert a.check() == []
    c = a.clean()
    assert c.full('X').shape == (R, LDX) and float(c.full('X')[:, CIN:].abs().max()) == 0.0 and c['X'].stride() == a['X'].stride()
    correct_layer(c)
    for name in ('Y', 'arg', 'stat'):
        assert torch.equal(a.result(name), c.result(name)), name
    assert float(a.result('stat')[2 * COUT]) == 100.0 + 2 * COUT  # the running sum it started from


def _one_behind_an_output(a):
    a.flat[torch.float32][a.offset('Y') + R * LDY] = 1.0


def _one_in_front_of_an_output(a):
    a.flat[torch.float32][a.offset('Y') - 1] = 1.0


def _into_a_pad_column(a):
    a.flat[torch.float32][a.offset('Y') + 2 * LDY + COUT] = 0.0


def _into_an_input(a):
    a['W'][1, 2] += 1.0


def _past_the_end_of_a_scratch(a):
    a.flat[torch.float64][a.offset('partial') + R * COUT] = 0.0


def _into_an_integer_guard(a):
    a.flat[torch.uint8][a.offset('arg') + R * COUT] = 1


def _statistics_slot_behind_the_last(a):
    a.flat[torch.float64][a.offset('stat') + 2 * COUT + 1] += 1.0


@pytest.mark.parametrize('plant,operand,words', [
    (_one_behind_an_output, 'Y', 'store behind the operand, element offset {}'.format(R * LDY)),
    (_one_in_front_of_an_output, 'Y', 'store in front of the operand, element offset -1'),
    (_into_a_pad_column, 'Y', 'store a pad column of the operand, element offset {} (row 2, column {})'.format(2 * LDY + COUT, COUT)),
    (_into_an_input, 'W', 'input changed at element offset {} (row 1, column 2)'.format(LDW + 2)),
    (_past_the_end_of_a_scratch, 'partial', 'store behind the operand, element offset {}'.format(R * COUT)),
    (_into_an_integer_guard, 'arg', 'store behind the operand, element offset {}'.format(R * COUT)),
    (_statistics_slot_behind_the_last, 'stat', 'store behind the operand, element offset {}'.format(2 * COUT + 1)),
])
def test_a_stray_store_is_reported_with_the_operand_and_the_offset(plant, operand, words):
    a = layer_arena()
    correct_layer(a)
    plant(a)
    found = a.check()
    assert len(found) == 1 and found[0].startswith(operand + ': ') and words in found[0], found


def test_a_pad_that_is_loaded_and_multiplied_by_zero_shows_in_the_result():
    """The mistake that X[:, Cin:] = 7.0 cannot see: the whole padded row against a zero-padded weight tile.  7 * 0 = 0, NaN * 0 = NaN."""
    a = layer_arena()
    correct_layer(a)
    w_tile = torch.zeros(COUT, LDX)
    w_tile[:, :CIN] = a['W'][:, :CIN]
    x_rows = a.flat[torch.float32].as_strided((R, LDX), (LDX, 1), a.offset('X'))  # the rows, pads included
    a['Y'][:, :COUT] = x_rows @ w_tile.t()
    found = a.check()
    assert len(found) == 1 and found[0].startswith("Y: result element (row 0, column 0) = offset 0 is the arena's NaN"), found
    # the same implementation on zero-padded separate allocations is indistinguishable from the correct one
    c = a.clean()
    correct_layer(c)
    assert torch.equal(c.full('X') @ w_tile.t(), c.result('Y'))


def test_an_unwritten_output_element_is_reported():
    a = layer_arena()
    correct_layer(a)
    a['Y'][R - 1, COUT - 1] = a.flat[torch.float32][0]  # as if the tail had skipped it: the entry value again
    found = a.check()
    assert len(found) == 1 and found[0].startswith("Y: result element (row {}, column {}) = offset {} is the arena's NaN (never written".format(
        R - 1, COUT - 1, (R - 1) * LDY + COUT - 1)), found


def test_a_nan_the_case_declares_legitimate_is_not_a_finding():
    a = layer_arena()
    correct_layer(a)
    a['Y'][0, 0] = float('inf')
    found = a.check()
    assert found == ['Y: result element (row 0, column 0) = offset 0 is non-finite'] and a.check(nan_ok=('Y',)) == []


def test_a_stray_accumulate_is_seen_because_the_guards_of_an_accumulated_operand_are_finite():
    """NaN + x is the same NaN bit for bit: behind a NaN guard the statistics flush that adds into slot 2C+1 would change nothing."""
    a = layer_arena()
    nan_guard = a.flat[torch.float32][a.offset('Y') - 1].clone()
    assert torch.equal((nan_guard + 1.0).view(torch.int32), nan_guard.view(torch.int32))
    assert float(a.flat[torch.float64][a.offset('stat') + 2 * COUT + 1]) == ACC_GUARD == float(a.flat[torch.float64][a.offset('stat') - 1])


def test_finite_guards_for_an_output_that_atomics_add_into():
    """finite=True: the guards and pads of a written output hold the finite sentinel (a stray += shows), its result region still the NaN."""
    a = Arena('cpu')
    a.out('grad', (3, 2), ld=4, finite=True).inp('stat_in', torch.ones(5, dtype=torch.float64), finite=True)
    a.build()
    f, o = a.flat[torch.float32], a.offset('grad')
    assert float(f[o - 1]) == ACC_GUARD == float(f[o + 2]) == float(f[o + 12]) and torch.isnan(a['grad']).all()
    assert float(a.flat[torch.float64][a.offset('stat_in') - 1]) == ACC_GUARD
    a['grad'].zero_()
    assert a.check() == []
    f[o + 12] += 1.0   # the scatter-add that lands one row behind the gradient
    assert a.check() == ['grad: store behind the operand, element offset 12 (row 3, column 0) from its start']
