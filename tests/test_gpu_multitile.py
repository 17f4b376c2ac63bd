"""The N>1 path on real hardware, as far as a 1-GPU box allows: 2 ranks share GPU 0, every
exchange point of the step goes through the C-ABI hook and extpom_amd.halo (edges staged through
the host over gloo, because RCCL wants one GPU per rank), and the owned cells of both tiles must
equal the single-tile CPU oracle bit for bit -- in an x split, a y split and a 2x2 split (4 ranks:
corner cells travel through both exchange phases)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["x", "y", "xy"])
def test_two_tiles_on_one_gpu_match_single_tile_oracle(split):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_worker.py"), split], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_four_tiles_with_the_4th_order_pressure_gradient():
    """npg = 2 on a 2x2 split: baropg_mcc's extra ghost column / row travel through the order hook"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_worker.py"), "xy", "npg2"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("args", [["xy", "transport"], ["xy", "npg2", "transport"], ["xy", "wide"], ["x", "wide"], ["y", "npg2", "wide"]])
def test_library_exchange_and_wide_halo_external_mode(args):
    """pomgpu_set_transport (the library packs / moves / unpacks at every exchange point; the mover here stages
    through the host because the ranks share one GPU) and pomgpu_set_wide_external (one wide exchange per internal
    step instead of six narrow ones per external substep): owned cells equal the single-tile oracle bit for bit"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_worker.py")] + args, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("args", [["xy", "wide"], ["y", "wide"]])
def test_wide_halo_mode_with_two_substeps_per_pass(args):
    """the extended tile of the wide-halo mode under k_ext_march2 (two external substeps per pass over memory; its default on tiles
    as large as those of a 2-GPU split of the bench grid, forced here): owned cells equal the single-tile oracle bit for bit"""
    env = dict(os.environ, POMGPU_EXT_PAIR="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_worker.py")] + args, capture_output=True,
                       text=True, timeout=900, env=env)
    assert r.returncode == 0 and "TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "k_ext_pair" in r.stdout, r.stdout[-1500:]         # the path under test did run (the worker prints rank 0's kernel list)


@pytest.mark.gpu
@pytest.mark.parametrize("args", [["y4", "wide"], ["y4", "transport"]])
def test_whole_row_tiles_the_default_split(args):
    """1 x 4 whole-row tiles (decomp.choose_tile_grid's choice, what bench.py --gpus N runs): the two inner tiles are extended on both
    sides in the wide-halo mode (the shrinking row window of their external substeps, the balanced XCD order of ragged tiles), have two
    neighbours and no corner messages: owned cells equal the single-tile oracle bit for bit"""
    env = dict(os.environ, POM_TILES_GRID="72x150x12")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_worker.py")] + args, capture_output=True,
                       text=True, timeout=900, env=env)
    assert r.returncode == 0 and "TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_full_size_decomposition_invariance_whole_rows_and_baselines_2x4():
    """The property the reference itself guarantees, at the size north_star is stated on: 2048x1536x50 as ONE
    tile, as 1 x 4 whole-row tiles (bench.py's default split) and as the 2 x 4 tiles BASELINE configs[3] runs on 8 GPUs (1025 x 386,
    the north row of tiles trimmed to 384 rows, every tile with three or five live neighbours incl. the diagonal ones:
    parallel_mpi.f:54-65,82-119,96-103) -- library exchange with corner messages, wide-halo external mode, rounds on the second stream --
    GPU against GPU on one device, 50 internal steps: every owned cell of every COMMON array that is not scratch carries the same
    bits.  With steps 1-3 of the single-tile run pinned to the oracle at this size (test_config4_2048x1536x50_full_size) this is
    what carries the pin beyond a few steps, and over the multi-tile path."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_threads.py"), "2048x1536x50", "1x4,2x4", "50"], capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0 and "TILES-THREADS-OK 2048x1536x50 1x4 50" in r.stdout and "TILES-THREADS-OK 2048x1536x50 2x4 50" in r.stdout, \
        r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_config2_grid_as_baselines_2x4_tiles():
    """BASELINE configs[2] as it is worded: the closed basin 1024x1024x40 on a 2 x 4 tile decomposition (tiles 513 x 258, the north
    row of tiles trimmed to jm = 256 of 258), eight contexts on one GPU, 20 internal steps against the single tile: every owned
    cell of every COMMON array that is not scratch carries the same bits.  The single tile of this grid is pinned to the oracle
    for steps 1-3 (test_restart_and_determinism_properties_1024x1024x40)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_threads.py"), "1024x1024x40", "2x4", "20"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TILES-THREADS-OK 1024x1024x40 2x4 20" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "(513, 256," in r.stdout and "(513, 258," in r.stdout, r.stdout[-3000:]      # the trimmed north row of tiles did run


@pytest.mark.gpu
@pytest.mark.parametrize("args", [["x", "rccl"], ["xy", "rccl"], ["y", "npg2", "rccl"]])
def test_rccl_between_distinct_ranks_one_gpu_each(args):
    """bench.py's N > 1 path as a parity test: rank r on GPU r, the library's RCCL transport (main and side stream, both
    communicators) and the wide-halo external mode between DIFFERENT ranks; owned cells equal the single-tile oracle bit
    for bit.  Needs one GPU per rank: skipped on the one-GPU boxes the builder had (the path between two distinct ranks
    has not run anywhere yet -- DESIGN.md section 7)."""
    import torch
    need = 4 if args[0] == "xy" else 2
    if torch.cuda.device_count() < need:                      # counting devices does not initialise the GPU in this process
        pytest.skip(f"needs {need} GPUs, this box has {torch.cuda.device_count()}")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_worker.py")] + args, capture_output=True,
                       text=True, timeout=900, env=env)
    assert r.returncode == 0 and "TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_rccl_transport_on_a_periodic_single_rank():
    """The RCCL mover itself, as far as one GPU allows: a communicator of one rank whose tile is its own western
    and eastern neighbour (a periodic channel), so every exchange point and the wide exchange send and receive real
    ncclSend / ncclRecv messages on the kernels' stream.  The same configuration with a device-copy callback mover
    must give bit-identical fields."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_rccl_self.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "RCCL-SELF-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("args", [["seamount_2x2", "hook"], ["seamount_2x2", "transport"], ["seamount_2x2_npg2", "transport"], ["island_2x2", "transport"],
                                  ["seamount_2x2_isplit10", "wide"], ["seamount_2x2_isplit10_npg2", "wide"]])
def test_hip_tiles_equal_the_references_own_mpi_run(args):
    """four ranks on GPU 0, the reference's own tile size (34 x 26 on 65x49x21): every restart-list field of every rank,
    ghost cells included, hashes to what the REFERENCE left on that rank of a four-process MPICH run
    (tests/golden/tiles_65x49x21_2x2.json) -- with the per-point hooks, the library exchange and the wide-halo mode"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tiles_golden_worker.py")] + args, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "TILES-GOLDEN-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- the fourth case (extpom_amd.cases: archipelago): land on the seams, in the ghost lines, in the wide-halo rim and on the open edges, a
# curved grid.  The device's lane shifts and LDS slabs carry dum, dvm, dt, cor and the curvature coefficients between lanes and rows; the
# emulated build reads them from memory, so these runs are the authority for them (tests/test_host_logic.py asserts the land per split)
@pytest.mark.gpu
@pytest.mark.parametrize("args", [["x"], ["y"], ["xy"], ["x", "transport"], ["y", "transport"], ["xy", "transport"], ["x", "wide"], ["y", "wide"], ["xy", "wide"],
                                  ["xy", "npg2", "wide"]], ids="-".join)
def test_archipelago_tiles_on_one_gpu_match_single_tile_oracle(args):
    """2 x 1, 1 x 2 and 2 x 2 tiles of 97x61x16 with the per-point hooks, the library exchange and the wide-halo external mode;
    baropg_mcc once: owned cells equal the single-tile oracle bit for bit"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_worker.py")] + args + ["case=archipelago"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("args", [["xy"], ["xy", "transport"], ["xy", "wide"]], ids="-".join)
def test_off_default_constants_on_archipelago_tiles(args):
    """every run constant off its default (tests/off_default.py: four different rf*, both biases, alpha, the ramp ...) on 2 x 2 tiles of
    97x61x16 with the per-point hooks, the library exchange and the wide-halo external mode: the tile-edge kernels state the filter, alpha
    and the boundary radiation on their own, and an edge factor applied on a side that has a neighbour shows.  Owned cells equal the
    single-tile oracle under the same constants bit for bit"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_worker.py")] + args + ["constants=off", "case=archipelago"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_archipelago_whole_row_tiles():
    """1 x 4 whole-row tiles (72x150x12), wide-halo mode: the two inner tiles extended on both sides, land in their rims"""
    env = dict(os.environ, POM_TILES_GRID="72x150x12")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_worker.py"), "y4", "wide", "case=archipelago"], capture_output=True,
                       text=True, timeout=900, env=env)
    assert r.returncode == 0 and "TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_archipelago_256x192x50_as_2x4_tiles_event_ordered_mover():
    """the asynchronous (event-ordered) mover of gpu_tiles_threads.py, rounds on the second stream really beside the kernels: 2 x 4 tiles
    of 256x192x50, 10 internal steps, every owned cell against the single tile (which the reference digests pin,
    test_gpu_reproduces_reference_digests_archipelago_kb50)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_threads.py"), "256x192x50", "2x4", "10", "case=archipelago"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TILES-THREADS-OK 256x192x50 2x4 10" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("args", [["archipelago_2x2", "hook"], ["archipelago_2x2", "transport"], ["archipelago_2x2", "wide"]])
def test_hip_tiles_equal_the_references_own_mpi_run_archipelago(args):
    """as test_hip_tiles_equal_the_references_own_mpi_run, on the reference's four-process run of the fourth case
    (tests/golden/tiles_archipelago_65x49x21_2x2.json): ghost cells included"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tiles_golden_worker.py")] + args, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "TILES-GOLDEN-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
