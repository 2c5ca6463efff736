"""The layouts of a Newton-KKT plan, stated once as tables in csrc/kkt_plan.hpp (MODEL_ARENA, FIRST_ORDER_ARENA,
THETA_ARENA, walked by walk_arena; vector_layout): tests/cpp/test_kkt_plan.cpp prints every offset and length for a
fixed list of dimension sets, on the host.  Held here against the oracle's tables (kkt_oracle_model_offset,
kkt_oracle_vector_offset, kkt_oracle_theta_offset) and, for the first-order arena, against a walk written from the
order include/sip_kkt_amd.h documents."""
import subprocess

from oracle.kkt import KKTDims, KKTOracle
from tests import reference_kkt_problems as rk

NODE_BLOCKS = {"model": 3, "first": 5, "theta": 4}   # the blocks before these are per node, the others per edge
PER_EDGE_TABLES = (1, 4, 6)                          # SIP_KKT_X_CONTROL, SIP_KKT_Y_EDGE_C, SIP_KKT_Z_EDGE


def _chain(n, m, T, cn, gn, cT, gT, ce, ge):
    return KKTDims(list(range(T)), list(range(1, T + 1)), [n] * (T + 1), [m] * T, node_c=[cn] * T + [cT],
                   node_g=[gn] * T + [gT], edge_c=[ce] * T, edge_g=[ge] * T)


DIM_SETS = [
    rk.newton_kkt_dims(4, 1, 3),
    _chain(5, 3, 4, 1, 2, 3, 2, 2, 3),
    _chain(3, 2, 1, 1, 0, 2, 1, 1, 2),
    KKTDims([], [], [3], [], node_c=[2], node_g=[1]),
    # the non-uniform chain and the branching tree (root 2, a state of dimension zero) of tests/test_gpu_first_order.py
    KKTDims(list(range(6)), list(range(1, 7)), [4, 6, 5, 3, 6, 4, 5], [2, 3, 1, 2, 3, 2], node_c=[1, 0, 2, 0, 1, 0, 2],
            node_g=[0, 2, 0, 1, 0, 0, 3], edge_c=[1, 2, 0, 1, 1, 0], edge_g=[2, 0, 1, 1, 0, 2]),
    KKTDims(parents=[2, 0, 2, 0], children=[0, 3, 1, 4], state_dims=[3, 5, 4, 0, 2], control_dims=[2, 0, 3, 1],
            node_c=[1, 0, 2, 1, 0], node_g=[0, 2, 1, 0, 3], edge_c=[1, 0, 2, 1], edge_g=[2, 1, 0, 1], root=2),
]


def _first_order_walk(d, p):
    """include/sip_kkt_amd.h, "first-order arena": node i followed by edge i;
    node i : f (1) | df_dx (n_i) | df_dtheta (p) | c (c_i) | g (g_i)
    edge e : f (1) | df_dx (np) | df_du (m) | df_dtheta (p) | dyn_res (nc) | c (ce) | g (ge)"""
    off, at = {}, 0
    for i in range(d.N):
        for block, size in enumerate((1, d.sd[i], p, d.ncd[i], d.ngd[i])):
            off[block, i] = at
            at += size
        if i < d.E:
            sizes = (1, d.sd[d.parents[i]], d.cd[i], p, d.sd[d.children[i]], d.ecd[i], d.egd[i])
            for block, size in enumerate(sizes, start=5):
                off[block, i] = at
                at += size
    return off, at


def _parse(text):
    """[(header, {"dims": {...}, "len": {...}, "off": {(arena, block, index): value}})] per printed set."""
    sets = []
    for line in text.splitlines():
        word = line.split()
        if word[0] == "set":
            sets.append((line, {"dims": {}, "len": {}, "off": {}}))
        elif word[0] == "dims":
            sets[-1][1]["dims"][word[1]] = [int(v) for v in word[2:]]
        elif word[0] == "len":
            sets[-1][1]["len"] = {k: int(v) for k, v in zip(word[1::2], word[2::2])}
        else:
            assert word[0] == "off", line
            sets[-1][1]["off"][word[1], int(word[2]), int(word[3])] = int(word[4])
    return sets


def test_kkt_plan_layouts():
    import __graft_entry__ as entry
    entry.build_oracle()
    exe = entry.build_kkt_plan_test()
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, (proc.stdout[-3000:], proc.stderr[-3000:])
    printed = _parse(proc.stdout)
    assert len(printed) == 2 * len(DIM_SETS)
    for k, (header, got) in enumerate(printed):
        base, p = DIM_SETS[k // 2], (0, 3)[k % 2]
        d = KKTDims(base.parents, base.children, base.sd, base.cd, base.ncd, base.ngd, base.ecd, base.egd,
                    root=base.root, theta_dim=p)
        assert header.endswith(f"| theta {p} | root {d.root}"), header
        assert got["dims"] == dict(parents=d.parents, children=d.children, sd=d.sd, cd=d.cd, ncd=d.ncd, ngd=d.ngd,
                                   ecd=d.ecd, egd=d.egd), header
        oracle = KKTOracle(d)
        fo, fo_len = _first_order_walk(d, p)
        assert got["len"] == dict(x=d.x_dim, y=d.y_dim, z=d.z_dim, model=d.model_len, first=fo_len,
                                  theta=d.theta_len), header
        want = {}
        for arena, count, offset in (("model", 12, oracle.model_offset), ("first", 12, lambda b, i: fo[b, i]),
                                    ("theta", 10 if p else 0, oracle.theta_offset)):
            for block in range(count):
                for i in range(d.N if block < NODE_BLOCKS[arena] else d.E):
                    want[arena, block, i] = offset(block, i)
        for table in range(7):
            for i in range(d.E if table in PER_EDGE_TABLES else d.N):
                want["vector", table, i] = oracle.vector_offset(table, i)
        assert got["off"] == want, header
        oracle.close()
