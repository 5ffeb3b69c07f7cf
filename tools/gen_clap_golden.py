"""Generate tests/golden/clap_text_g5.npz and tests/golden/clap_text_state_dict_spec.json on the CPU.

The expected values come from `transformers.RobertaModel` (eager attention) built with roberta-base's config.json numbers
(vocab 50265, 514 positions, type vocab 1, LayerNorm eps 1e-5, exact-erf GELU, pad id 1), loaded with
lass_amd.synthetic.make_clap_text_state_dict, run on ids padded to 512 as the reference tokenizes them; the CLAP head
(Linear -> ReLU -> Linear, F.normalize; CLAP/open_clip/model.py:432,454,732-751) is restated below.  Two weight sets: 12
layers (roberta-base) and 2 layers.  The GPU tests regenerate the same weights from the stored seeds.

    python tools/gen_clap_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lass_amd import clap_text, synthetic  # noqa: E402

SETS = [(synthetic.SEED + 8, 12), (synthetic.SEED + 9, 2)]  # (seed, layers)
LENGTHS = [2, 5, 9, 17, 24, 31, 77, 130, 300, 512]
PAD_IN_MASK_ROW = 4   # this row holds id 1 (the pad id) at a position inside its mask
HOLE_ROW = 5          # this row's mask has a 0 inside the caption (trimming is exact for any mask with mask[:,0] == 1)


def make_ids(seed: int = 99):
    rng = np.random.Generator(np.random.PCG64(seed))
    n, S = len(LENGTHS), clap_text.MAX_LENGTH
    ids = np.full((n, S), clap_text.PAD_ID, dtype=np.int64)
    mask = np.zeros((n, S), dtype=np.int64)
    for i, L in enumerate(LENGTHS):
        ids[i, 0] = 0                                        # <s>
        ids[i, 1:L - 1] = rng.integers(3, clap_text.VOCAB, L - 2)
        ids[i, L - 1] = 2                                    # </s>
        mask[i, :L] = 1
    ids[PAD_IN_MASK_ROW, 7] = clap_text.PAD_ID
    mask[HOLE_ROW, 11] = 0
    return ids, mask


def roberta(layers: int):
    from transformers import RobertaConfig, RobertaModel

    cfg = RobertaConfig(vocab_size=clap_text.VOCAB, hidden_size=768, num_hidden_layers=layers, num_attention_heads=12,
                        intermediate_size=3072, hidden_act="gelu", max_position_embeddings=clap_text.MAX_POSITIONS,
                        type_vocab_size=1, layer_norm_eps=clap_text.LAYER_NORM_EPS, pad_token_id=1, bos_token_id=0,
                        eos_token_id=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cfg._attn_implementation = "eager"
    return RobertaModel(cfg).eval()


def run(seed: int, layers: int, ids: np.ndarray, mask: np.ndarray):
    sd = synthetic.make_clap_text_state_dict(seed, layers)
    m = roberta(layers)
    pre = "model.text_branch."
    missing, unexpected = m.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(pre)},
                                            strict=False)
    assert not unexpected and all(k.endswith(("position_ids", "token_type_ids")) for k in missing), (missing, unexpected)
    with torch.no_grad():
        pooler = m(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).pooler_output
        t = lambda k: torch.from_numpy(sd["model.text_projection." + k])  # noqa: E731
        x = torch.relu(pooler @ t("0.weight").T + t("0.bias")) @ t("2.weight").T + t("2.bias")
        emb = torch.nn.functional.normalize(x, dim=-1)
    return pooler.numpy().astype(np.float32), emb.numpy().astype(np.float32)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ids, mask = make_ids()
    out = {"lengths": np.asarray(LENGTHS, dtype=np.int64), "input_ids": ids, "attention_mask": mask,
           "seeds": np.asarray([s for s, _ in SETS], dtype=np.int64), "layers": np.asarray([l for _, l in SETS], dtype=np.int64)}
    for seed, layers in SETS:
        pooler, emb = run(seed, layers, ids, mask)
        out[f"pooler_l{layers}"] = pooler
        out[f"embed_l{layers}"] = emb
        print(f"layers {layers}: |pooler| max {np.abs(pooler).max():.3f}, embed[0,:4] {emb[0, :4]}")
    golden = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(golden, "clap_text_g5.npz"), **out)
    spec = {k: list(s) for k, s, _ in clap_text.param_specs(12)}
    with open(os.path.join(golden, "clap_text_state_dict_spec.json"), "w") as f:
        json.dump(spec, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
