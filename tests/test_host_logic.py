"""CPU: host-side logic of the product (no kernels are launched): integer paths bit-exact against the golden
vectors captured from the reference, optimizer grouping / LR schedule, arena ordering, window geometry tables,
and that the C-ABI library loads and exports every symbol declared in include/lavender_hip.h."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch


def _g(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def test_library_exports_every_declared_symbol():
    from lavender_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "lavender_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(lav_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(_lib.lib, name), f"{name} declared in lavender_hip.h but not exported"
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert _lib.lib.lav_abi_version() == _lib.ABI_VERSION == 7
    # ... and nothing else: every exported text symbol of the shared object is a declared entry point of one of the two headers
    import subprocess
    hdr2 = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "lavender_pipeline.h")).read(), flags=re.S)
    declared |= set(re.findall(r"\b(lav_[a-z0-9_]+)\s*\(", hdr2))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    assert exported == declared, exported ^ declared


def test_argument_errors_are_reported_not_thrown():
    from lavender_amd import _lib
    rc = _lib.lib.lav_gemm_bf16(None, 7, 1, 1, 1, None, 8, None, 8, None, 8, None, 1)
    assert rc < 0 and b"layout" in _lib.lib.lav_last_error()


@pytest.mark.parametrize("seed", [88, 0, 1])
@pytest.mark.parametrize("BX", [(2, 33), (8, 32), (32, 32)])
def test_masking_bit_exact(golden_dir, seed, BX):
    from lavender_amd.pretrain_mlm import masking
    g = _g(golden_dir, "ints")
    B, X = BX
    tin = torch.from_numpy(g[f"masking_s{seed}_B{B}_X{X}_in"]).clone()
    torch.manual_seed(seed)
    out = masking(tin, (tin != 0).long(), (101, 102, 0, 103))
    assert (out["txt"].numpy() == g[f"masking_s{seed}_B{B}_X{X}_txt"]).all()
    assert (out["ans_mtm"].numpy() == g[f"masking_s{seed}_B{B}_X{X}_ans"]).all()


def test_vtm_pairs_known_answer():
    from lavender_amd.pretrain_mlm import vtm_pairs
    np.random.seed(88)
    vi, ti, tr = vtm_pairs(4, 4)
    assert ti.reshape(4, 4)[:, 1:].tolist() == [[2, 3, 1], [3, 0, 2], [3, 1, 0], [0, 1, 2]]
    assert vi.tolist() == [i for i in range(4) for _ in range(4)]
    assert tr.reshape(4, 4)[:, 0].all() and not tr.reshape(4, 4)[:, 1:].any()


def test_param_groups_match_reference(golden_dir):
    from lavender_amd.arena import param_group_of
    g = _g(golden_dir, "agent")
    for i in range(4):
        for n in g[f"group{i}"].tolist():
            assert param_group_of(n) == i, n


def test_lr_schedule_matches_reference(golden_dir):
    from lavender_amd.agent import WarmupLinearLR

    class Opt:
        param_groups = [dict(lr=2e-5)]
    o = Opt()
    sch = WarmupLinearLR(o, 100)
    lrs = []
    for _ in range(110):
        lrs.append(o.param_groups[0]["lr"])
        sch.step()
    np.testing.assert_allclose(lrs, _g(golden_dir, "ints")["lr_max_iter100_lr2e-5"], rtol=1e-12)
    assert lrs[0] == 1e-8                                         # first optimizer step runs at the min_lr floor


def test_state_dict_keys_match_reference(golden_dir):
    from tests.helpers import Tok, make_args
    from lavender_amd import LAVENDER_Pretrain_MLM
    t = _g(golden_dir, "tiny2l_b2")
    m = LAVENDER_Pretrain_MLM(make_args("tiny", "b2l", 2), Tok())
    ours = {k: str(tuple(v.shape)) for k, v in m.state_dict().items()}
    ref = dict(zip(t["keys"].tolist(), t["shapes"].tolist()))
    assert ours == ref
    assert len(list(m.named_parameters())) == 221            # decoder.bias tied to predictions.bias


def test_state_dict_keys_of_the_other_callers_match_reference(golden_dir):
    """LAVENDER_Pretrain (fc.1 / fc.3 score head, no emb_task), LAVENDER_Retrieval_MLM and its eval subclass: same
    state_dict keys as the reference classes (captured by tests/golden/make_goldens_variants.py)."""
    from tests.helpers import Tok, make_args
    from lavender_amd import LAVENDER_Pretrain, LAVENDER_Retrieval_MLM, LAVENDER_RetrievalMlmEval
    ts = _g(golden_dir, "ts_micro_b5")
    m = LAVENDER_Pretrain(make_args("micro", "micro", 5), Tok())
    assert {k: str(tuple(v.shape)) for k, v in m.state_dict().items()} == dict(zip(ts["keys"].tolist(), ts["shapes"].tolist()))
    rt = _g(golden_dir, "retr_micro_b3")
    for cls in (LAVENDER_Retrieval_MLM, LAVENDER_RetrievalMlmEval):
        assert set(cls(make_args("micro", "micro", 3), Tok()).state_dict()) == set(rt["keys"].tolist())


def test_arena_order_groups_qkv():
    from lavender_amd.arena import _order
    names = []
    for n in ("query", "key", "value"):
        names += [f"trsfr.layer.0.attention.self.{n}.weight", f"trsfr.layer.0.attention.self.{n}.bias"]
    named = [("a.weight", 0)] + [(n, 0) for n in names] + [("b.bias", 0)]
    got = [n for n, _ in _order(named)]
    pre = "trsfr.layer.0.attention.self."
    assert got == ["a.weight"] + [pre + f"{n}.weight" for n in ("query", "key", "value")] + \
        [pre + f"{n}.bias" for n in ("query", "key", "value")] + ["b.bias"]


def test_get_window_size(golden_dir):
    from lavender_amd.video_swin import get_window_size
    g = _g(golden_dir, "ints")
    for c, o in zip(g["gws_in"], g["gws_out"]):
        w, s = get_window_size(tuple(c[0]), tuple(c[1]), tuple(c[2]))
        assert (list(w), list(s)) == (list(o[0]), list(o[1]))


@pytest.mark.parametrize("win", [(8, 7, 7), (8, 12, 12)])
def test_relative_position_index(golden_dir, win):
    from lavender_amd.video_swin import relative_position_index
    g = _g(golden_dir, "ints")
    idx = relative_position_index(win).numpy().astype(np.int64)
    assert hashlib.sha256(idx.tobytes()).hexdigest() == str(g["rpi_" + "x".join(map(str, win)) + "_sha"])


@pytest.mark.parametrize("case", [(5, 56, 56, (5, 7, 7), (0, 3, 3)), (5, 14, 14, (5, 7, 7), (0, 3, 3)),
                                  (4, 14, 14, (2, 7, 7), (1, 3, 3)), (5, 21, 21, (5, 7, 7), (0, 3, 3)),
                                  (5, 7, 7, (5, 7, 7), (0, 0, 0))])
def test_window_tables_reproduce_roll_partition_and_mask(golden_dir, case):
    """tok table == roll(-shift) + window_partition of a token-index tensor (video_swin.py:82-86,218-227);
    type/region tables reproduce compute_mask (video_swin.py:290-305) bit-exactly."""
    from lavender_amd.hip import window_tables
    from oracle import lavender_ref as R
    D, H, W, win, sh = case
    N = win[0] * win[1] * win[2]
    t = window_tables(torch.device("cpu"), D, H, W, win, sh)
    ids = torch.arange(D * H * W, dtype=torch.float32).view(1, D, H, W, 1)
    rolled = torch.roll(ids, (-sh[0], -sh[1], -sh[2]), (1, 2, 3)) if any(sh) else ids
    ref = R.partition(rolled, win).squeeze(-1).long()
    assert (t["tok"][:, :N].long() == ref).all() and (t["tok"][:, N:] == -1).all()
    if any(sh):
        reg = t["region"].long()[t["wtype"].long()][:, :N]
        mine = torch.where(reg[:, None, :] != reg[:, :, None], -100.0, 0.0)
        assert torch.equal(mine, R.shift_mask(D, H, W, win, sh))
        g = _g(golden_dir, "ints")
        tag = f"mask_{D}_{H}_{W}_" + "x".join(map(str, win)) + "_" + "x".join(map(str, sh)) + "_sha"
        if tag in g.files:
            assert hashlib.sha256(np.packbits((mine != 0).numpy()).tobytes()).hexdigest() == str(g[tag])


def test_no_cpu_path():
    from tests.helpers import Tok, make_args
    from lavender_amd import LAVENDER_Pretrain_MLM
    m = LAVENDER_Pretrain_MLM(make_args("micro", "micro", 2), Tok())
    with pytest.raises(RuntimeError, match="MI355X"):
        m.arena()


def test_args_json_overlay(tmp_path):
    import json
    from lavender_amd.args import parse_with_config
    cfg = tmp_path / "a.json"
    cfg.write_text(json.dumps({"size_batch": 24, "size_frame": 4, "type": "pretrain", "lr": 2e-5}))
    a = parse_with_config(["--config", str(cfg), "--size_batch", "32"])
    assert a.size_batch == 32 and a.size_frame == 4 and a.type == "pretrain" and a.lr == 2e-5   # CLI > JSON > default


def test_bench_algorithmic_flops_match_the_survey_table():
    """bench.flops_per_sample is the closed form of SURVEY.md section 8d; its table gives 428.9 / 80.7 / 1956.0 / 574.6
    GFLOP forward per sample for configs 2, 1, 4 and 5 -- the figure roofline / step_mfma_frac are computed from."""
    import bench as B
    assert abs(B.flops_per_sample() / 1e9 - 428.9) < 0.1
    assert abs(B.flops_per_sample(E=96, depths=(2, 2, 6, 2), layers=2, n_seq=3) / 1e9 - 80.7) < 0.1
    assert abs(B.flops_per_sample(E=192, win=(8, 12, 12), S=384) / 1e9 - 1956.0) < 0.1
    assert abs(B.flops_per_sample(X=26, n_seq=8) / 1e9 - 574.6) < 0.1


def test_checkpoint_contract_round_trip(tmp_path):
    """LAVENDER_Base.load_ckpt (model.py:352-429): a state_dict written the way Agent_Base.save_model writes it loads back
    key for key; foreign task-head keys and missing heads are tolerated (non-strict), a missing file is a no-op."""
    import torch
    from tests.helpers import Tok, make_args
    from lavender_amd import LAVENDER_Pretrain_MLM, LAVENDER_Pretrain
    torch.manual_seed(1)
    a = LAVENDER_Pretrain_MLM(make_args("micro", "micro", 2), Tok())
    path = str(tmp_path / "ckpt_violet_pretrain_1.pt")
    torch.save({k: v.cpu() for k, v in a.state_dict().items()}, path)
    torch.manual_seed(2)
    b = LAVENDER_Pretrain_MLM(make_args("micro", "micro", 2), Tok())
    assert not torch.equal(a.enc_img.swin.layers[0].blocks[0].mlp.fc1.weight, b.enc_img.swin.layers[0].blocks[0].mlp.fc1.weight)
    b.load_ckpt(path)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    # the pre-trained MLM checkpoint into the task-specific model: its score head stays at init, emb_task is unexpected
    torch.manual_seed(3)
    c = LAVENDER_Pretrain(make_args("micro", "micro", 2), Tok())
    fc0 = c.fc[1].weight.detach().clone()
    c.load_ckpt(path)
    assert torch.equal(c.fc[1].weight, fc0) and torch.equal(c.trsfr.layer[0].output.dense.weight, a.trsfr.layer[0].output.dense.weight)
    c.load_ckpt(str(tmp_path / "does_not_exist.pt"))
    c.load_ckpt('')


def test_bench_spawns_its_own_ranks_and_refuses_a_wrong_world_size():
    """`python bench.py --gpus N` without a launcher must start N ranks itself (not label a 1-rank run as N GPUs), and a
    launcher world size that contradicts --gpus must fail loudly.  --selftest-launch stops after the rendezvous + all-reduce
    (gloo: the GPUs are hidden from the ranks, so the check is the same on a host with one GPU or none)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--selftest-launch"], capture_output=True, text=True,
                       timeout=240, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["world_observed"] == 2
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--selftest-launch"], capture_output=True, text=True,
                       timeout=120, env={**env, "WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout)


def test_bench_dump_outputs_writes_the_same_float_arrays_for_the_same_state(tmp_path):
    """bench.py --dump-outputs: the last step's losses and a seeded sample of the parameters as float .npy files within 64 MB,
    identical for identical model state (two builds are compared file by file)."""
    import types
    import bench
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.Linear(200, 7))
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    got = []
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), m, types.SimpleNamespace(dp=None), {"mtm": torch.tensor(1.5), "vtm": torch.tensor(0.25)}, 0)
        got.append({f: np.load(tmp_path / run / f) for f in sorted(os.listdir(tmp_path / run))})
    assert sorted(got[0]) == ["loss_mtm.npy", "loss_vtm.npy", "param_sample.npy"]
    assert all(v.dtype in (np.float32, np.float64) for v in got[0].values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in got[0]) <= 64 << 20
    assert got[0]["loss_mtm.npy"] == 1.5 and got[0]["loss_vtm.npy"] == 0.25
    assert np.isin(got[0]["param_sample.npy"], flat).all() and len(got[0]["param_sample.npy"]) > 0.9 * flat.size
    assert all(np.array_equal(got[0][f], got[1][f]) for f in got[0])
    bench.dump_outputs(str(tmp_path / "rank1"), m, types.SimpleNamespace(dp=None), {"mtm": torch.tensor(1.5)}, 1)
    assert not os.path.exists(tmp_path / "rank1")


def test_bench_plain_run_measures_only_the_headline():
    """A plain bench.py run stops at its result line: the reference loop, the roofline sampling steps, the CPU baseline and the
    child runs (side workloads, A/B, 1-rank RCCL) come with --full only, where the --no-* switches drop single legs as before."""
    import bench

    def legs(*argv, world=1):
        return bench.full_legs(bench.arg_parser().parse_args(list(argv)), world)
    everything = ["ref_loop", "roofline", "cpu_baseline", "children"]
    for argv in ([], ["--gpus", "1", "--steps", "20", "--warmup", "5"], ["--workload", "cfg4"], ["--input", "tsv"], ["--force-dp"],
                 ["--dump-outputs", "d"]):
        assert legs(*argv) == [] and legs(*argv, world=8) == [], argv
    assert legs("--full") == everything
    assert legs("--full", world=8) == ["ref_loop", "roofline"]
    assert legs("--full", "--no-ref-loop") == everything[1:]
    assert legs("--full", "--no-cpu-baseline") == ["ref_loop", "roofline"]
    assert legs("--full", "--no-side-workloads") == everything[:3]
    assert legs("--full", "--workload", "cfg4") == ["ref_loop", "roofline"]
    assert legs("--full", "--workload", "cfg5") == ["roofline"]
    assert legs("--full", "--input", "tsv") == ["roofline", "cpu_baseline"]


def test_hf_checkpoint_loader_renames_legacy_layernorm_keys_and_ties_the_decoder(tmp_path):
    """Stock bert-base-uncased files name LayerNorm parameters gamma / beta and omit the tied cls.predictions.decoder.weight;
    `from_pretrained` (model.py:100-102, main_pretrain_mlm.py:46-48) fixes both up, so must load_hf_state."""
    from lavender_amd.bert import BertConfigLite, BertEmbeddings, BertOnlyMLMHead, load_hf_into, load_hf_state
    cfg = BertConfigLite(vocab_size=50, hidden_size=64, num_attention_heads=1, intermediate_size=128, max_position_embeddings=16)
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    sd = {"bert.embeddings.word_embeddings.weight": r(50, 64), "bert.embeddings.position_embeddings.weight": r(16, 64),
          "bert.embeddings.token_type_embeddings.weight": r(2, 64), "bert.embeddings.LayerNorm.gamma": r(64),
          "bert.embeddings.LayerNorm.beta": r(64), "bert.embeddings.position_ids": torch.arange(16)[None],
          "cls.predictions.bias": r(50), "cls.predictions.transform.dense.weight": r(64, 64), "cls.predictions.transform.dense.bias": r(64),
          "cls.predictions.transform.LayerNorm.gamma": r(64), "cls.predictions.transform.LayerNorm.beta": r(64)}
    torch.save(sd, tmp_path / "pytorch_model.bin")
    emb = BertEmbeddings(cfg)
    res = load_hf_into(emb, load_hf_state(str(tmp_path), [("bert.embeddings.", "")]), "embeddings")
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(emb.LayerNorm.weight.data, sd["bert.embeddings.LayerNorm.gamma"])
    assert torch.equal(emb.LayerNorm.bias.data, sd["bert.embeddings.LayerNorm.beta"])
    head = BertOnlyMLMHead(cfg)
    res = load_hf_into(head, load_hf_state(str(tmp_path), [("cls.", "")]), "head")
    assert not res.missing_keys
    assert torch.equal(head.predictions.decoder.weight.data, sd["bert.embeddings.word_embeddings.weight"])
    assert torch.equal(head.predictions.transform.LayerNorm.weight.data, sd["cls.predictions.transform.LayerNorm.gamma"])


def test_pipeline_library_exports_and_host_side(golden_dir):
    """include/lavender_pipeline.h: every declared entry is exported; the host-only entries (TSV reader, JPEG header) work
    without a GPU and agree with the CPU restatement of dataset.py:40-46 / PIL."""
    import re
    import numpy as np
    from lavender_amd import _lib, data as D
    from oracle import pipeline_ref as PR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "lavender_pipeline.h")).read()
    declared = set(re.findall(r"\b(lav_[a-z0-9_]+)\s*\(", hdr)) - {"lav_last_error"}
    assert declared == set(_lib.PIPELINE_EXPORTS), declared ^ set(_lib.PIPELINE_EXPORTS)
    tsvp, idxp = os.path.join(golden_dir, "msrvtt_2rows.tsv"), os.path.join(golden_dir, "msrvtt_2rows.lineidx")
    for idx in (idxp, None):                               # with the reference's .lineidx, and indexing the lines itself
        tsv = D.TsvFile(tsvp, idx)
        assert len(tsv) == 2
        for r in range(2):
            ref = PR.read_row(tsvp, tsv.offset(r))
            assert tsv.seek(tsv.offset(r)) == ref
            for b in tsv.fields(tsv.offset(r))[1:]:
                assert D.jpeg_size(b) == (320, 240)
        tsv.close()
    g = np.load(os.path.join(golden_dir, "pipeline_frames.npz"))
    import base64
    for name in g["syn_names"].tolist():
        h, w = g[f"syn_{name}_rgb"].shape[:2]
        assert D.jpeg_size(base64.b64encode(g[f"syn_{name}_jpg"].tobytes())) == (w, h)
    # frame choice and resize geometry (dataset.py:188-216, torchvision Resize(int))
    import random
    from tests.helpers import Tok
    ds = D.Dataset_Base(type("A", (), dict(size_img=224, img_transform=["img_rand_crop"], size_txt=8))(), "train", 4, Tok())
    for n in range(1, 12):
        for cfg in (1, 3, 4, 5):
            ds.size_frame = cfg
            random.seed(n * 7 + cfg)
            a = ds.temporal_sample(list(range(n)), random_sample=True)
            random.seed(n * 7 + cfg)
            assert a == PR.temporal_sample(list(range(n)), cfg, True)
            assert ds.temporal_sample(list(range(n))) == PR.temporal_sample(list(range(n)), cfg)
    assert D.resized_size(320, 240, 224) == (298, 224) and D.resized_size(240, 320, 224) == (224, 298) and D.resized_size(7, 7, 224) == (224, 224)


def test_loader_sampler_orders_match_torch_samplers():
    """get_dl's index order (dataset.py:279-287): DistributedSampler(shuffle = train) / RandomSampler / SequentialSampler of torch,
    reproduced without a Dataset object -- same indices for the same seeds, epochs, ranks."""
    import torch
    from torch.utils.data import DistributedSampler, RandomSampler, SequentialSampler
    from lavender_amd.data import _Sampler

    class DS:
        def __init__(self, n): self.n = n
        def __len__(self): return self.n
        def __getitem__(self, i): return i
    for n in (1, 7, 10, 33):
        for world in (1, 2, 4):
            for rank in range(world):
                for train in (True, False):
                    for epoch in (0, 3):
                        ref = DistributedSampler(DS(n), num_replicas=world, rank=rank, shuffle=train)
                        ref.set_epoch(epoch)
                        s = _Sampler(n, train, True, rank, world)
                        s.set_epoch(epoch)
                        assert s.indices() == list(ref), (n, world, rank, train, epoch)
        torch.manual_seed(11)
        a = list(RandomSampler(DS(n)))
        torch.manual_seed(11)
        assert _Sampler(n, True, False).indices() == a
        assert _Sampler(n, False, False).indices() == list(SequentialSampler(DS(n)))


def test_gemm_epilogue_pack_format_matches_the_c_struct():
    """hip.gemm fills lav_gemm_epilogue with one struct.pack_into (lavender_amd/hip.py:_EPI_PACK): every field must land where the
    ctypes declaration of the struct (= the C layout, include/lavender_hip.h) puts it, with the value it was given."""
    import ctypes as C
    import struct
    from lavender_amd import _lib as L, hip as K
    fields = [f[0] for f in L.GemmEpilogue._fields_]
    assert tuple(fields) == K._EPI_FIELDS
    vals = []
    for i, (name, ct) in enumerate(L.GemmEpilogue._fields_):
        if ct is L.f32:
            vals.append(0.5 + i)
        elif ct is L.vp:
            vals.append(0x1000_0000_0000 + 16 * i)
        elif ct is L.u32:
            vals.append(0xF000_0000 + i)
        else:
            vals.append(1000 + i)
    raw = C.create_string_buffer(C.sizeof(L.GemmEpilogue))
    K._EPI_PACK.pack_into(raw, 0, *vals)
    st = C.cast(raw, C.POINTER(L.GemmEpilogue)).contents
    for name, v in zip(fields, vals):
        got = getattr(st, name)
        assert (got or 0) == v, (name, got, v)
    assert K._EPI_PACK.size <= C.sizeof(L.GemmEpilogue) < K._EPI_PACK.size + 8          # only tail padding may differ


def test_stage_descriptor_pack_formats_match_the_c_structs():
    """lav_bert_layer_desc / lav_bert_layer_bwd_desc / lav_swin_block_desc / lav_swin_block_bwd_desc are filled with one struct.pack_into each
    (lavender_amd/hip.py:_BL_FWD_PACK / _BL_BWD_PACK / _SB_FWD_PACK / _SB_BWD_PACK):
    every value must land in the field the ctypes declaration (= include/lavender_hip.h) gives it."""
    import ctypes as C
    from lavender_amd import _lib as L, hip as K

    def flat_fields(st, prefix=()):
        out = []
        for name, ct in st._fields_:
            if isinstance(ct, type) and issubclass(ct, C.Structure):
                out += flat_fields(ct, prefix + (name,))
            else:
                out.append((prefix + (name,), ct))
        return out

    for st, packer in ((L.BertLayerDesc, K._BL_FWD_PACK), (L.BertLayerBwdDesc, K._BL_BWD_PACK), (L.SwinBlockDesc, K._SB_FWD_PACK),
                       (L.SwinBlockBwdDesc, K._SB_BWD_PACK)):
        fields = flat_fields(st)
        vals = [(0.25 + i) if ct is L.f32 else (0x2000_0000_0000 + 8 * i) if ct is L.vp else (0xE000_0000 + i) if ct is L.u32 else (700 + i)
                for i, (_, ct) in enumerate(fields)]
        raw = C.create_string_buffer(C.sizeof(st))
        packer.pack_into(raw, 0, *vals)
        obj = C.cast(raw, C.POINTER(st)).contents
        for (path, _), v in zip(fields, vals):
            got = obj
            for part in path:
                got = getattr(got, part)
            assert (got or 0) == v, (path, got, v)
