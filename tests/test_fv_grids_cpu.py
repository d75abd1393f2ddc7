"""The one device cache of solvers/fv/grids.py, on devices that need no GPU ("cpu", and "meta" as a second one)."""
import numpy as np
import torch


def test_cached_tables_share_one_upload_per_key_and_device():
    from solvers.fv.grids import cached_tables, device_index
    built = []

    def build():
        built.append(1)
        return np.arange(3.0), np.asfortranarray(np.arange(6.0).reshape(2, 3))

    key = ("test_fv_grids_cpu", 3, 1.0, 1.5)
    first, again = cached_tables(key, "cpu", build), cached_tables(list(key), torch.device("cpu"), build)
    assert len(built) == 1 and len(first) == 2 and all(a is b for a, b in zip(first, again))
    assert all(t.dtype == torch.float64 and t.is_contiguous() and t.device.type == "cpu" for t in first)
    assert np.array_equal(first[1].numpy(), np.arange(6.0).reshape(2, 3))
    for q in range(len(key)):                                      # any element of the key
        other = list(key)
        other[q] = "another table" if q == 0 else key[q] + 1
        got = cached_tables(other, "cpu", build)
        assert all(a is not b for a, b in zip(first, got))
    assert len(built) == 1 + len(key)
    meta = cached_tables(key, "meta", build)                       # the device
    assert meta[0].device.type == "meta" and meta[0] is not first[0] and len(built) == 2 + len(key)
    assert cached_tables(key, "meta", build)[0] is meta[0] and cached_tables(key, "cpu", build)[0] is first[0]
    assert device_index(torch.device("cuda:3")) == 3 and device_index(torch.device("cpu")) == 0


def test_the_getters_keep_their_tables_apart():
    from solvers.fv import grids as G
    lam, S = G.sine_eig(5, "cpu")
    assert G.sine_eig(5, "cpu")[1] is S and G.sine_eig(6, "cpu")[1] is not S
    assert G.wall_eig(5, "cpu")[1] is not S                        # equal arguments, another table
    assert np.array_equal(S.numpy(), G.sine_eig_host(5)[1]) and np.array_equal(lam.numpy(), G.sine_eig(5)[0])
    tx = G.transfer_axis(8, 1.0, 1.5, "cpu")
    assert G.transfer_axis(8, 1.0, 1.5, "cpu") is tx and G.transfer_axis(8, 2.0, 1.5, "cpu") is not tx
    assert G.wall_stretched_axis(8, 1.0, 1.5, "cpu") is not tx and tx.numel() == 4 * 8 + 2
    table, lam, Q = G.grid_axis(8, 1.0, 1.5, "cpu")
    assert G.grid_axis(8, 1.0, 1.5, "cpu", rho=1.0)[2] is Q and G.grid_axis(8, 1.0, 1.5, "cpu", rho=2.0)[2] is not Q
    assert np.array_equal(table.numpy(), tx.numpy()[8:])           # [h | d | g] behind the centres
    px, py = G.separable_tables(8, 12, 1.0, 1.0, 1.5, "cpu")
    assert G.separable_tables(8, 12, 1.0, 1.0, 1.5, "cpu")[0] is px and G.separable_tables(12, 8, 1.0, 1.0, 1.5, "cpu")[0] is not px
    assert (px.numel(), py.numel()) == (8 * 10, 12 * 14)
