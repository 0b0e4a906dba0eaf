"""K16 in the engine against the torch formulation (KGC_LOGITS_KERNEL=0): greedy requests
that together use all five fields, more requests than slots so later ones re-enter used slots.

One rounding step cannot differ between the paths here (same fp32 operations, one rounding,
and every frequency_penalty is dyadic so a contracted multiply-add rounds the same), but the
tiny random model has near-ties that rounding upstream may break either way.  So each request
carries a logit_bias ladder its penalties cannot climb down in 16 tokens, and the torch path
checks that every processed row's top-two gap exceeds one bf16 step at every position.  That
makes the token comparison blind to small value errors, so the second test compares the two
paths' processed logits bit for bit, before and after an update.
"""
import pytest
import torch

from kubernetes_gpu_cluster_amd.engine.logits_processor import LogitsProcessor
from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams

pytestmark = pytest.mark.gpu


def _params():
    _ladder = lambda base, step: {base + i: 40.0 - step * i for i in range(4)}   # noqa: E731
    kw = dict(temperature=0, max_tokens=16, ignore_eos=True)
    return [SamplingParams(presence_penalty=0.5, frequency_penalty=0.25,
                           logit_bias=_ladder(10, 8.0), **kw),
            SamplingParams(repetition_penalty=1.3, logit_bias=_ladder(20, 8.0), **kw),
            SamplingParams(logit_bias={**_ladder(30, 8.0), "11": -100, 900: 1.7}, **kw),
            SamplingParams(min_p=0.1, logit_bias=_ladder(40, 8.0), **kw),
            SamplingParams(presence_penalty=-0.5, frequency_penalty=0.125, repetition_penalty=0.9,
                           logit_bias=_ladder(50, 8.0), min_p=0.05, **kw),
            SamplingParams(frequency_penalty=0.25, repetition_penalty=1.1,
                           logit_bias=_ladder(60, 8.0), **kw)]


def _generate(kernel: bool, monkeypatch):
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLM
    monkeypatch.setenv("KGC_LOGITS_KERNEL", "1" if kernel else "0")
    steps = []       # torch path: per step, the smallest top-two gap in bf16 steps of the leader
    if not kernel:
        torch_apply = LogitsProcessor.apply

        def spy(self, logits, rows):
            torch_apply(self, logits, rows)
            v = logits[[r[0] for r in rows]].float().topk(2).values
            steps.append(((v[:, 0] - v[:, 1]) / torch.exp2(v[:, 0].abs().log2().floor() - 7)).min())
        monkeypatch.setattr(LogitsProcessor, "apply", spy)
    llm = LLM("tiny-llama", device="cuda", dtype="bfloat16", random_init=True, seed=3,
              max_model_len=256, max_num_seqs=4, max_num_batched_tokens=256)
    g = torch.Generator().manual_seed(11)
    outs = []
    for _ in range(2):                     # the second batch finds every slot used
        prompts = [torch.randint(3, 1000, (5 + i,), generator=g).tolist() for i in range(6)]
        outs += [o.output_token_ids for o in llm.generate(prompts, _params())]
    proc = llm.engine.executor.runner.processor
    assert proc.kernel == kernel and (proc.stats is not None) == kernel \
        and (proc.counts is not None) != kernel
    llm.shutdown()
    assert kernel or min(float(x) for x in steps) > 1.0, "a top-two gap within one bf16 step"
    return outs


def test_engine_tokens_equal_torch_path(gpu, monkeypatch):
    got, want = _generate(True, monkeypatch), _generate(False, monkeypatch)
    assert all(len(o) == 16 for o in got)
    assert got == want


def test_processor_paths_agree_bitwise(gpu):
    V, rows = 1024, [(i, 6 - i, p) for i, p in enumerate(_params())]
    g = torch.Generator().manual_seed(0)
    for scale in (0.5, 6.0):
        logits = (torch.randn(7, V, generator=g) * scale).to(torch.bfloat16).to(gpu)
        outs = []
        for kernel in (True, False):
            proc = LogitsProcessor(8, V, gpu)
            proc.kernel = kernel
            for i, slot, p in rows:
                proc.init_slot(slot, [1, 2, 3, 4 + i], [5, 5, 6 + i, 900, 10 + 10 * i])
            first, second = logits.clone(), logits.clone()
            proc.apply(first, rows)
            proc.update(rows, torch.arange(7, device=gpu) + 5)
            proc.apply(second, list(rows))
            outs.append(torch.stack([first, second]).view(torch.int16))
        assert torch.equal(outs[0], outs[1]), (scale, (outs[0] != outs[1]).nonzero()[:8].tolist())
