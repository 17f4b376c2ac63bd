"""The restore rate as a field on an MI355X: the checks of tests/restore_rate_checks.py with the product library against
tests/restore_rate_expect.py's restatement, the reference's recorded digests (tests/golden/restore_rate.json) and the oracle, bit for bit;
the fp32 study builds against the fp64 result rounded once."""
import pytest

import restore_rate_checks as C
from extpom_amd import lib

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("shape,kind,chunk_kb,layout,nrec", [
    ((8, 8, 2, 6), "d", None, "unlimited", 4), ((8, 8, 5, 6), "f", None, "fixed", 4), ((20, 17, 5, 6), "d", 1, "unlimited", 4),
    ((20, 17, 5, 6), "f", 1, "unlimited", 1), ((20, 17, 5, 6), "d", None, "none", 1), ((20, 17, 5, 6), "f", None, "fixed", 1),
    ((65, 49, 33, 21), "d", 1, "unlimited", 4)], ids=str)
def test_rate_file_equals_the_setter_fed_the_mapped_records(tmp_path, shape, kind, chunk_kb, layout, nrec):
    C.file_equals_setter(LIB, tmp_path, shape, kind=kind, chunk_kb=chunk_kb, layout=layout, nrec=nrec, version=1 if layout == "fixed" else 2)


def test_a_map_that_goes_below_zero_is_the_references(tmp_path):
    C.file_equals_setter(LIB, tmp_path, (65, 49, 33, 21), layout="none", nrec=1, steep=True)


def test_rate_file_beside_t_and_s_from_the_clim_file(tmp_path):
    C.ts_from_the_clim_file(LIB, tmp_path)


def test_tiles_equal_the_global_map_cut_to_their_window(tmp_path):
    C.tiles(LIB, tmp_path)


@pytest.mark.parametrize("case", ["archipelago", "seamount"])
def test_four_steps_after_a_load_equal_the_oracle_in_all_three_forms(tmp_path, case):
    C.steps_after_a_load(LIB, tmp_path, case)


def test_a_rate_mirror_written_from_outside_the_step_is_used():
    C.a_written_mirror_is_used(LIB)


def test_every_new_refusal_leaves_the_state_as_it_was(tmp_path):
    C.refusals(LIB, tmp_path)


def test_without_a_rate_source_restore_interior_is_the_references():
    C.no_rate_source_is_the_reference(LIB)


@pytest.mark.parametrize("path", [lib.LIBPATH_F32, lib.LIBPATH_F32A], ids=["f32", "f32a"])
def test_fp32_builds_round_the_rate_once(tmp_path, path):
    C.f32_rounds_once(path, tmp_path)
