"""World-size-2 gloo rehearsal of the custom error table's broadcast (distributed.broadcast_error_tables):
rank 0's table is what every rank runs, and a rank whose own table differs raises with both digests."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T_POS = [[(ma + 2 * mb + 3) % 4 for mb in range(8)] for ma in range(8)]
T_SGN = [[v - 1 for v in row] for row in T_POS]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Op(torch.nn.Module):
    """A stand-in operator: what the broadcast reads is the custom_approx_params dict."""

    def __init__(self, params):
        super().__init__()
        self.custom_approx_params = params


def _worker(rank, ws, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        from fp8_quantization_amd.distributed import broadcast_error_tables
        from fp8_quantization_amd.error_tables import table_digest
        out = {}
        # 1. rank 0 holds the table (two operators share one spec), rank 1 none: rank 1 takes rank 0's
        shared = dict(mant_width=3, **({"error_table": T_POS} if rank == 0 else {}))
        model = torch.nn.Sequential(_Op(shared), _Op(shared), _Op(dict(mant_width=2)))
        broadcast_error_tables(model, src=0)
        t = model[0].custom_approx_params["error_table"]
        out["adopted"] = torch.as_tensor(t).tolist()
        out["same_object"] = model[1].custom_approx_params["error_table"] is t
        out["untouched"] = "error_table" not in model[2].custom_approx_params
        # 2. both hold the same table (one as a list, one as a tensor): nothing raises, nothing changes
        spec = T_POS if rank == 0 else torch.tensor(T_POS)
        model = torch.nn.Sequential(_Op(dict(mant_width=3, error_table=spec)))
        broadcast_error_tables(model, src=0)
        out["kept"] = model[0].custom_approx_params["error_table"] is spec
        # 3. rank 1's own table differs: it raises naming both digests, and rank 0 does not wait forever
        model = torch.nn.Sequential(_Op(dict(mant_width=3, error_table=T_POS if rank == 0 else T_SGN)))
        try:
            broadcast_error_tables(model, src=0)
            out["differs"] = None
        except ValueError as e:
            out["differs"] = str(e)
        # 4. rank 1 holds a table where rank 0 has none
        model = torch.nn.Sequential(_Op(dict(mant_width=3, **({"error_table": T_SGN} if rank == 1 else {}))))
        try:
            broadcast_error_tables(model, src=0)
            out["extra"] = None
        except ValueError as e:
            out["extra"] = str(e)
        out["digests"] = (table_digest(torch.tensor(T_POS)), table_digest(torch.tensor(T_SGN)))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_error_table_broadcast():
    ws = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, ws, port, q)) for r in range(ws)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(ws))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    d_pos, d_sgn = res[0]["digests"]
    for rank in range(ws):
        r = res[rank]
        assert r["adopted"] == T_POS and r["same_object"] and r["untouched"] and r["kept"]
        assert r["differs"] is not None and r["extra"] is not None  # every rank raises, none hangs
    assert d_sgn in res[1]["differs"] and d_pos in res[1]["differs"] and "rank 1" in res[1]["differs"]
    assert d_sgn in res[1]["extra"] and "none" in res[1]["extra"]
