"""CPU tier of the force family's kernel-name table (csrc/su3_force.hip: force_entry_kernel_name, which
l2q_kernel_name answers the force entry points from): for every force entry and l2q_su3_flow_stage, at force_tile 2, 5
and 7, on lattices that between them reach the thread-per-link, slice-resident, plaquette-sharing and LDS-tiled
kernels, the 'force + plaquette' composite and the upper-plane refusals, the library gives the answers recorded from
it before the force family got a file, a launcher and a name function of its own.  Nothing is launched."""
import pytest

ENTRIES = ('l2q_su3_force', 'l2q_su3_force_kick', 'l2q_su3_force_action', 'l2q_su3_force_upper',
           'l2q_su3_force_action_upper', 'l2q_su3_flow_stage')

# (force_tile, lattice) -> the answer for each of ENTRIES
RECORDED = {
    (2, (8, 8, 8, 8)): (
        'su3_force_slice_kernel<false, 128, 0, 2>',
        'su3_force_slice_kernel<true, 128, 2, 1>',
        'su3_force_slice_kernel<false, 128, 0, 2> + su3_plaq_slice_kernel<true>',
        '',
        '',
        'su3_force_slice_kernel<true, 128, 2, 1> + su3_expm_mul_kernel<false, false>',
    ),
    (2, (16, 16, 16, 16)): (
        'su3_force_slice_kernel<false, 128, 0, 2>',
        'su3_force_slice_kernel<true, 128, 2, 1>',
        'su3_force_slice_kernel<false, 128, 0, 2> + su3_plaq_slice_kernel<false>',
        '',
        '',
        'su3_force_slice_kernel<true, 128, 2, 1> + su3_expm_mul_kernel<false, false>',
    ),
    (2, (2, 4, 4, 4)): (
        'su3_force_tile_kernel<false, 2>',
        'su3_force_tile_kernel<true, 2>',
        'su3_force_tile_kernel<false, 2> + su3_plaq_kernel<2>',
        '',
        '',
        'su3_force_tile_kernel<true, 2> + su3_expm_mul_kernel<false, false>',
    ),
    (2, (4, 8, 8, 8)): (
        'su3_force_slice_kernel<false, 128, 0, 2>',
        'su3_force_slice_kernel<true, 128, 2, 1>',
        'su3_force_slice_kernel<false, 128, 0, 2> + su3_plaq_slice_kernel<true>',
        '',
        '',
        'su3_force_slice_kernel<true, 128, 2, 1> + su3_expm_mul_kernel<false, false>',
    ),
    (2, (1, 3, 2, 5)): (
        'su3_force_tile_kernel<false, 2>',
        'su3_force_tile_kernel<true, 2>',
        'su3_force_tile_kernel<false, 2> + su3_plaq_kernel<2>',
        '',
        '',
        'su3_force_tile_kernel<true, 2> + su3_expm_mul_kernel<false, false>',
    ),
    (2, (3, 5, 2, 7)): (
        'su3_force_tile_kernel<false, 2>',
        'su3_force_tile_kernel<true, 2>',
        'su3_force_tile_kernel<false, 2> + su3_plaq_kernel<2>',
        '',
        '',
        'su3_force_tile_kernel<true, 2> + su3_expm_mul_kernel<false, false>',
    ),
    (2, (2, 2, 8, 8)): (
        'su3_force_slice_kernel<false, 128, 0, 2>',
        'su3_force_slice_kernel<true, 128, 2, 1>',
        'su3_force_slice_kernel<false, 128, 0, 2> + su3_plaq_slice_kernel<true>',
        '',
        '',
        'su3_force_slice_kernel<true, 128, 2, 1> + su3_expm_mul_kernel<false, false>',
    ),
    (5, (8, 8, 8, 8)): (
        'su3_force_link_kernel<0, 6>',
        'su3_force_link_kernel<1, 6>',
        'su3_force_link_action_kernel<6>',
        'su3_force_link_kernel<4, 6>',
        'su3_force_link_action_upper_kernel<6>',
        'su3_force_link_kernel<1, 6> + su3_expm_mul_kernel<false, false>',
    ),
    (5, (16, 16, 16, 16)): (
        'su3_force_link_kernel<0, 4>',
        'su3_force_link_kernel<1, 4>',
        'su3_force_link_action_kernel<4>',
        'su3_force_link_kernel<4, 4>',
        'su3_force_link_action_upper_kernel<4>',
        'su3_force_link_kernel<1, 4> + su3_expm_mul_kernel<false, false>',
    ),
    (5, (2, 4, 4, 4)): (
        'su3_force_link_kernel<0, 7>',
        'su3_force_link_kernel<1, 7>',
        'su3_force_link_action_kernel<7>',
        'su3_force_link_kernel<4, 7>',
        'su3_force_link_action_upper_kernel<7>',
        'su3_force_link_kernel<1, 7> + su3_expm_mul_kernel<false, false>',
    ),
    (5, (4, 8, 8, 8)): (
        'su3_force_link_kernel<0, 6>',
        'su3_force_link_kernel<1, 6>',
        'su3_force_link_action_kernel<6>',
        'su3_force_link_kernel<4, 6>',
        'su3_force_link_action_upper_kernel<6>',
        'su3_force_link_kernel<1, 6> + su3_expm_mul_kernel<false, false>',
    ),
    (5, (1, 3, 2, 5)): (
        'su3_force_tile_kernel<false, 2>',
        'su3_force_tile_kernel<true, 2>',
        'su3_force_tile_kernel<false, 2> + su3_plaq_kernel<2>',
        '',
        '',
        'su3_force_tile_kernel<true, 2> + su3_expm_mul_kernel<false, false>',
    ),
    (5, (3, 5, 2, 7)): (
        'su3_force_tile_kernel<false, 2>',
        'su3_force_tile_kernel<true, 2>',
        'su3_force_tile_kernel<false, 2> + su3_plaq_kernel<2>',
        '',
        '',
        'su3_force_tile_kernel<true, 2> + su3_expm_mul_kernel<false, false>',
    ),
    (5, (2, 2, 8, 8)): (
        'su3_force_link_kernel<0, 6>',
        'su3_force_link_kernel<1, 6>',
        'su3_force_link_action_kernel<6>',
        'su3_force_link_kernel<4, 6>',
        'su3_force_link_action_upper_kernel<6>',
        'su3_force_link_kernel<1, 6> + su3_expm_mul_kernel<false, false>',
    ),
    (7, (8, 8, 8, 8)): (
        'su3_force_plaq_kernel',
        'su3_force_link_kernel<1, 6>',
        'su3_force_plaq_kernel + su3_plaq_slice_kernel<true>',
        '',
        '',
        'su3_force_link_kernel<1, 6> + su3_expm_mul_kernel<false, false>',
    ),
    (7, (16, 16, 16, 16)): (
        'su3_force_link_kernel<0, 4>',
        'su3_force_link_kernel<1, 4>',
        'su3_force_link_action_kernel<4>',
        'su3_force_link_kernel<4, 4>',
        'su3_force_link_action_upper_kernel<4>',
        'su3_force_link_kernel<1, 4> + su3_expm_mul_kernel<false, false>',
    ),
    (7, (2, 4, 4, 4)): (
        'su3_force_link_kernel<0, 7>',
        'su3_force_link_kernel<1, 7>',
        'su3_force_link_action_kernel<7>',
        'su3_force_link_kernel<4, 7>',
        'su3_force_link_action_upper_kernel<7>',
        'su3_force_link_kernel<1, 7> + su3_expm_mul_kernel<false, false>',
    ),
    (7, (4, 8, 8, 8)): (
        'su3_force_plaq_kernel',
        'su3_force_link_kernel<1, 6>',
        'su3_force_plaq_kernel + su3_plaq_slice_kernel<true>',
        '',
        '',
        'su3_force_link_kernel<1, 6> + su3_expm_mul_kernel<false, false>',
    ),
    (7, (1, 3, 2, 5)): (
        'su3_force_tile_kernel<false, 2>',
        'su3_force_tile_kernel<true, 2>',
        'su3_force_tile_kernel<false, 2> + su3_plaq_kernel<2>',
        '',
        '',
        'su3_force_tile_kernel<true, 2> + su3_expm_mul_kernel<false, false>',
    ),
    (7, (3, 5, 2, 7)): (
        'su3_force_tile_kernel<false, 2>',
        'su3_force_tile_kernel<true, 2>',
        'su3_force_tile_kernel<false, 2> + su3_plaq_kernel<2>',
        '',
        '',
        'su3_force_tile_kernel<true, 2> + su3_expm_mul_kernel<false, false>',
    ),
    (7, (2, 2, 8, 8)): (
        'su3_force_plaq_kernel',
        'su3_force_link_kernel<1, 6>',
        'su3_force_plaq_kernel + su3_plaq_slice_kernel<true>',
        '',
        '',
        'su3_force_link_kernel<1, 6> + su3_expm_mul_kernel<false, false>',
    ),
}


@pytest.fixture
def native():
    from l2hmc import native
    native.load()
    yield native
    native.set_tuning('force_tile', 5)


def test_the_table_covers_what_it_says():
    assert len(RECORDED) == 3 * 7 and all(len(row) == len(ENTRIES) for row in RECORDED.values())
    names = ' '.join(n for row in RECORDED.values() for n in row)
    for kernel in ('su3_force_link_kernel<0,', 'su3_force_link_kernel<1,', 'su3_force_link_kernel<4,',
                   'su3_force_link_action_kernel', 'su3_force_link_action_upper_kernel', 'su3_force_slice_kernel<false',
                   'su3_force_slice_kernel<true', 'su3_force_plaq_kernel', 'su3_force_tile_kernel<false',
                   'su3_force_tile_kernel<true', ' + su3_plaq_kernel', ' + su3_plaq_slice_kernel<true>',
                   ' + su3_plaq_slice_kernel<false>'):
        assert kernel in names, kernel
    assert any(row[3] == '' and row[4] == '' for row in RECORDED.values())


@pytest.mark.parametrize('force_tile', (2, 5, 7))
def test_force_kernel_names_are_the_recorded_ones(native, force_tile):
    assert native.set_tuning('force_tile', force_tile) >= 0
    for (ft, lat), row in RECORDED.items():
        if ft != force_tile:
            continue
        for entry, want in zip(ENTRIES, row):
            assert native.kernel_name(entry, lat) == want, (force_tile, lat, entry)
