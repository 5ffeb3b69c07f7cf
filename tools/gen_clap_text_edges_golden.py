"""Generate tests/golden/clap_text_g7.npz on the CPU: the CLAP text tower at peaked attention and on every tile edge.

tests/golden/clap_text_g5.npz (tools/gen_clap_golden.py) draws every matrix from N(0, 0.02): the logits q.k/8 then have a
standard deviation of about 0.3, attention is an average over the caption, and a 1 % error in the softmax scale moves the
embedding by less than that fixture's bars.  This fixture uses synthetic.make_clap_text_state_dict(regime="peaked") - one
dominant key per query, GELU and tanh in their curved range - and captions whose real-token counts sit on and beside every
tile edge of text.hip: the 16-key online-softmax step, the 64-key LDS block / 64-query workgroup of k_attn, the 64-row tile of
k_gemm.  A third weight set has small embedding tables (vocab 300, 40 positions), which k_embed_ln takes at run time.

The expected values come from `transformers.RobertaModel` (eager attention, the config numbers of tools/gen_clap_golden.py) in
FLOAT64, with the CLAP head (Linear -> ReLU -> Linear, F.normalize) restated below.  Beside them the file records, per caption,
how far the same computation in float32 lies from the float64 one (`*_dev`, `embed_cosdev`: the tests' bars are 4 x the largest
of a set), and how far the float64 result moves when every layer's query weight and bias are multiplied by 1.01 (`*_mut`: a 1 %
error in the softmax scale).  Before anything is written the tool requires, for every set and both tensors, that the bar is
at most a quarter of the smallest mutation effect over the captions of at least two tokens (one token has a trivial softmax),
that the mean largest attention probability of the longest caption in layer 0 is at least 0.5, and that max |pooler| > 0.999.

    python tools/gen_clap_text_edges_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lass_amd import clap_text, synthetic  # noqa: E402

# (seed, layers, vocab, max_positions, caption set); every set is regime "peaked"
SETS = [(synthetic.SEED + 20, 2, clap_text.VOCAB, clap_text.MAX_POSITIONS, "full"),
        (synthetic.SEED + 21, 12, clap_text.VOCAB, clap_text.MAX_POSITIONS, "full"),
        (synthetic.SEED + 22, 1, 300, 40, "small")]
MUTATION = 1.01      # every layer's query weight and bias times this: the logits, hence the softmax scale, off by 1 %
BAR_FACTOR = 4       # bar = BAR_FACTOR x largest per-caption f32-vs-f64 deviation of the set
CAP_FRACTION = 0.25  # bar <= CAP_FRACTION x smallest mutation effect over captions of >= 2 tokens
MIN_PEAK = 0.5       # mean largest attention probability, longest caption, layer 0
MIN_SATURATION = 0.999

# real-token counts on and beside the edges: 16 (softmax step), 64 (LDS block, query block, GEMM row tile), 128, 512
COUNTS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 511, 512]
# rows after the plain ones: (span, position, what)
HOLE16_ROW, HOLE16_SPAN, HOLE16_POS = len(COUNTS), 40, 15       # mask 0 at position 15: packed key 15 is token 16
HOLE64_ROW, HOLE64_SPAN, HOLE64_POS = len(COUNTS) + 1, 200, 64  # mask 0 at position 64: the second LDS block starts at token 65
PAD_ROW, PAD_SPAN, PAD_POS = len(COUNTS) + 2, 260, 70           # the pad id inside the mask (its position id is the pad's)
IDS_ROW, IDS_SPAN, LAST_ID_POS = len(COUNTS) + 3, 250, 129      # second token id 3, token 129 the vocabulary's last row
SMALL_S, SMALL_COUNTS = 38, [1, 16, 17, 38]                     # 38: the longest that 40 positions admit


def _fill(ids, mask, i, span, rng, vocab):
    """Row i: <s>, span - 2 ids drawn from [3, vocab), </s>; a span of 1 is <s> alone."""
    ids[i, 0] = 0
    if span > 1:
        ids[i, 1:span - 1] = rng.integers(3, vocab, span - 2)
        ids[i, span - 1] = 2
    mask[i, :span] = 1


def make_captions(seed: int = 107):
    """(ids, mask, counts) of the full-size sets, (22, 512)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    spans = COUNTS + [HOLE16_SPAN, HOLE64_SPAN, PAD_SPAN, IDS_SPAN]
    ids = np.full((len(spans), clap_text.MAX_LENGTH), clap_text.PAD_ID, dtype=np.int64)
    mask = np.zeros_like(ids)
    for i, span in enumerate(spans):
        _fill(ids, mask, i, span, rng, clap_text.VOCAB)
    mask[HOLE16_ROW, HOLE16_POS] = 0   # the id under a hole stays: position ids count ids, not the mask
    mask[HOLE64_ROW, HOLE64_POS] = 0
    ids[PAD_ROW, PAD_POS] = clap_text.PAD_ID
    ids[IDS_ROW, 1] = 3
    ids[IDS_ROW, LAST_ID_POS] = clap_text.VOCAB - 1
    return ids, mask, mask.sum(1)


def make_small_captions(seed: int = 108, vocab: int = 300):
    """(ids, mask, counts) of the small-table set, (4, 38); ids 0, 2 and vocab - 1 all occur."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = np.full((len(SMALL_COUNTS), SMALL_S), clap_text.PAD_ID, dtype=np.int64)
    mask = np.zeros_like(ids)
    for i, span in enumerate(SMALL_COUNTS):
        _fill(ids, mask, i, span, rng, vocab)
    ids[1, 7] = vocab - 1
    ids[3, 20] = vocab - 1
    return ids, mask, mask.sum(1)


def roberta(layers: int, vocab: int, max_positions: int):
    from transformers import RobertaConfig, RobertaModel

    cfg = RobertaConfig(vocab_size=vocab, hidden_size=768, num_hidden_layers=layers, num_attention_heads=12,
                        intermediate_size=3072, hidden_act="gelu", max_position_embeddings=max_positions,
                        type_vocab_size=1, layer_norm_eps=clap_text.LAYER_NORM_EPS, pad_token_id=1, bos_token_id=0,
                        eos_token_id=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cfg._attn_implementation = "eager"
    return RobertaModel(cfg).eval()


def build(sd, layers: int, vocab: int, max_positions: int, dtype=torch.float64, query_scale: float = 1.0):
    """RobertaModel holding sd's text branch in `dtype`; query_scale multiplies every layer's query weight and bias (after the
    conversion, so a float64 model is mutated in float64)."""
    m = roberta(layers, vocab, max_positions)
    pre = "model.text_branch."
    missing, unexpected = m.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(pre)},
                                            strict=False)
    assert not unexpected and all(k.endswith(("position_ids", "token_type_ids")) for k in missing), (missing, unexpected)
    m = m.to(dtype)
    if query_scale != 1.0:
        with torch.no_grad():
            for layer in m.encoder.layer:
                layer.attention.self.query.weight.mul_(query_scale)
                layer.attention.self.query.bias.mul_(query_scale)
    return m


def forward(m, sd, ids: np.ndarray, mask: np.ndarray):
    """(pooler (N, 768), embedding (N, 512)) in m's dtype, as numpy."""
    dtype = next(m.parameters()).dtype
    with torch.no_grad():
        pooler = m(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).pooler_output
        t = lambda k: torch.from_numpy(sd["model.text_projection." + k]).to(dtype)  # noqa: E731
        x = torch.relu(pooler @ t("0.weight").T + t("0.bias")) @ t("2.weight").T + t("2.bias")
        emb = torch.nn.functional.normalize(x, dim=-1)
    return pooler.numpy(), emb.numpy()


def peakedness(m, ids: np.ndarray, mask: np.ndarray, row: int) -> float:
    """Mean over heads and real queries of the largest attention probability in layer 0, caption `row` alone."""
    with torch.no_grad():
        att = m(input_ids=torch.from_numpy(ids[row:row + 1]), attention_mask=torch.from_numpy(mask[row:row + 1]),
                output_attentions=True).attentions[0][0]            # (heads, S, S)
    real = torch.from_numpy(mask[row] != 0)
    return float(att[:, real][:, :, real].max(-1).values.mean())


def bars(g, si: int):
    """{tensor: bar} of set si from the recorded deviations; `g` is the fixture (or the dict about to be written)."""
    return {t: BAR_FACTOR * float(g[f"{t}_dev_s{si}"].max()) for t in ("embed", "pooler")}


def conditions(g, si: int, counts: np.ndarray):
    """The conditions a set must meet, as (description, holds) pairs - the tool refuses to write a fixture that misses one,
    tests/test_clap_text_cpu.py refuses a committed one."""
    multi = counts >= 2
    out = []
    for t, bar in bars(g, si).items():
        floor = float(g[f"{t}_mut_s{si}"][multi].min())
        out.append((f"set {si} {t}: bar {bar:.3e} <= {CAP_FRACTION} x smallest 1 % mutation effect {floor:.3e}",
                    bar <= CAP_FRACTION * floor))
    peak = float(g["peak"][si])
    out.append((f"set {si}: mean largest attention probability of the longest caption, layer 0: {peak:.3f} >= {MIN_PEAK}",
                peak >= MIN_PEAK))
    sat = float(np.abs(g[f"pooler_s{si}"]).max())
    out.append((f"set {si}: max |pooler| = 1 - {1 - sat:.3e} > {MIN_SATURATION}", sat > MIN_SATURATION))
    return out


def run_set(si: int, seed: int, layers: int, vocab: int, npos: int, ids, mask, counts):
    sd = synthetic.make_clap_text_state_dict(seed, layers, regime="peaked", vocab=vocab, max_positions=npos)
    m64 = build(sd, layers, vocab, npos)
    p64, e64 = forward(m64, sd, ids, mask)
    peak = peakedness(m64, ids, mask, int(np.argmax(counts)))
    del m64
    p32, e32 = forward(build(sd, layers, vocab, npos, torch.float32), sd, ids, mask)
    pm, em = forward(build(sd, layers, vocab, npos, query_scale=MUTATION), sd, ids, mask)
    cos = (e32.astype(np.float64) * e64).sum(1) / np.linalg.norm(e32.astype(np.float64), axis=1) / np.linalg.norm(e64, axis=1)
    return {f"pooler_s{si}": p64, f"embed_s{si}": e64,
            f"pooler_dev_s{si}": np.abs(p32 - p64).max(1), f"embed_dev_s{si}": np.abs(e32 - e64).max(1),
            f"embed_cosdev_s{si}": np.maximum(1 - cos, 0.0),
            f"pooler_mut_s{si}": np.abs(pm - p64).max(1), f"embed_mut_s{si}": np.abs(em - e64).max(1)}, peak


def _fmt(a) -> str:
    return " ".join(f"{v:.2e}" for v in a)


def generate():
    full, small = make_captions(), make_small_captions()
    out = {"input_ids": full[0], "attention_mask": full[1], "counts": full[2],
           "input_ids_small": small[0], "attention_mask_small": small[1], "counts_small": small[2],
           "seeds": np.asarray([s[0] for s in SETS], dtype=np.int64), "layers": np.asarray([s[1] for s in SETS], dtype=np.int64),
           "vocab": np.asarray([s[2] for s in SETS], dtype=np.int64),
           "max_positions": np.asarray([s[3] for s in SETS], dtype=np.int64),
           "small_tables": np.asarray([s[4] == "small" for s in SETS]), "peak": np.zeros(len(SETS))}
    for si, (seed, layers, vocab, npos, which) in enumerate(SETS):
        ids, mask, counts = small if which == "small" else full
        while True:
            res, peak = run_set(si, seed, layers, vocab, npos, ids, mask, counts)
            out.update(res)
            out["peak"][si] = peak
            out["layers"][si] = layers
            checks = conditions(out, si, counts)
            if which == "small" and layers == 1 and not all(ok for _, ok in checks):
                print(f"set {si}: 1 layer misses a condition, trying 2 layers")
                layers = 2
                continue
            break
        for t in ("embed", "pooler"):
            print(f"set {si} ({layers} layers, vocab {vocab}, {npos} positions) {t}: f32-vs-f64 deviation per caption "
                  f"{_fmt(out[f'{t}_dev_s{si}'])}; 1 % mutation effect per caption {_fmt(out[f'{t}_mut_s{si}'])}")
        print(f"set {si}: 1 - cosine of the f32 embedding {_fmt(out[f'embed_cosdev_s{si}'])}")
        for text, ok in checks:
            print(("ok   " if ok else "FAIL ") + text)
        if not all(ok for _, ok in checks):
            raise SystemExit(f"set {si} misses a condition: nothing written")
    return out


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = generate()
    path = os.path.join(ROOT, "tests", "golden", "clap_text_g7.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
