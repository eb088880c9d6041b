"""Drop-in entry points for callers of the reference's ``code_base/`` scripts (``run_single.py`` & co).

Same names, arguments and return values as ``code_base/arithmetic.py`` (``encode_arithmetic`` :78-217,
``decode_arithmetic`` :220-373) and ``code_base/sample.py`` (``sample`` :6-55), running on the HIP coder with
a KV-cached batched GPT-2 (PyTorch-ROCm); ``encode_huffman`` / ``decode_huffman`` (``huffman_baseline.py``) and
``get_bins`` / ``encode_block`` / ``decode_block`` (``block_baseline.py``) are served the same way.  ``model`` is
a Hugging Face GPT-2 (``GPT2LMHeadModel``), an already built :class:`~neuralsteganography_amd.lm.arithmetic.HipArithmeticLM`, or any batched-logits LM with
the ``prefill``/``step`` protocol; ``enc`` is the tokenizer (``encode``/``decode``).  ``device`` is accepted
for signature compatibility (the coder always runs on the current GPU).

Batched forms (``*_batch``) take lists of messages / texts and run them as one lockstep batch -- the point of
the build; the single-message functions are the batched ones at B = 1.

Behaviour notes (DESIGN.md "Deviations"):
* statistics (avg_NLL, avg_KL, words_per_bit, avg_Hq) are float64 values from fp32 device sums, within
  2e-5 relative of the reference's; tokens and bits are bit-exact;
* the '<eos>' stop of ``arithmetic.py:207-210`` is applied on a 16-token decoded tail per stream;
* ``sample`` draws with a counter-based generator (``seed``; torch.multinomial's stream is not
  reproducible), and also runs ``topk <= 0`` (every id), which the reference's ``sample.py:39`` cannot.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

_PROVIDERS: Dict[int, object] = {}


def _provider(model, enc, logits_dtype: str = "f32"):
    from .lm.arithmetic import HipArithmeticLM

    if isinstance(model, HipArithmeticLM):
        if enc is not None:
            model.tokenizer = enc
        return model
    key = (id(model), id(enc), logits_dtype)
    lm = _PROVIDERS.get(key)
    if lm is None:
        if hasattr(model, "prefill") and hasattr(model, "step"):
            lm = HipArithmeticLM.from_batched(model, enc, logits_dtype=logits_dtype)
        else:
            lm = HipArithmeticLM(model, enc, logits_dtype=logits_dtype)
        _PROVIDERS[key] = lm
    return lm


def _quality(temp, precision, topk, finish_sent=False):
    return {"temp": float(temp), "precision": int(precision), "topk": int(topk), "finish_sent": bool(finish_sent)}


def split_double_newlines(inp: List[int]) -> List[int]:
    """``decode_arithmetic``'s fix-up (arithmetic.py:233-242): token 628 ("\\n\\n") becomes 198, 198."""
    out: List[int] = []
    for t in inp:
        if t == 628:
            out += [198, 198]
        else:
            out.append(int(t))
    return out


def encode_arithmetic_batch(model, enc, messages: Sequence[Sequence[int]], context: Sequence[int],
                            finish_sent: bool = False, device: str = "cuda", temp: float = 1.0,
                            precision: int = 16, topk: int = 50000, stop_text: Optional[str] = "<eos>"
                            ) -> List[Tuple[List[int], float, float, float, float]]:
    """B messages (bit lists) -> per message ``(tokens, avg_NLL, avg_KL, words_per_bit, avg_Hq)``."""
    _ = device
    lm = _provider(model, enc)
    toks, stats = lm.encode_batch([list(m) for m in messages], list(context)[-1022:],
                                  quality=_quality(temp, precision, topk, finish_sent), return_stats=True,
                                  stop_text=stop_text)
    return [(t, s["avg_NLL"], s["avg_KL"], s["words_per_bit"], s["avg_Hq"]) for t, s in zip(toks, stats)]


def encode_arithmetic(model, enc, message: Sequence[int], context: Sequence[int], finish_sent: bool = False,
                      device: str = "cuda", temp: float = 1.0, precision: int = 16, topk: int = 50000):
    """``code_base/arithmetic.py:78`` -- returns ``(output, avg_NLL, avg_KL, words_per_bit, avg_Hq)``."""
    return encode_arithmetic_batch(model, enc, [message], context, finish_sent=finish_sent, device=device,
                                   temp=temp, precision=precision, topk=topk)[0]


def decode_arithmetic_batch(model, enc, texts: Sequence[str], context: Sequence[int], device: str = "cuda",
                            temp: float = 1.0, precision: int = 16, topk: int = 50000) -> List[List[int]]:
    """B cover texts -> the bit list each decodes to (every emitted bit; the caller truncates)."""
    _ = device
    lm = _provider(model, enc)
    token_lists = [split_double_newlines(list(enc.encode(t))) for t in texts]
    return lm.decode_tokens_repair(token_lists, list(context)[-1022:], quality=_quality(temp, precision, topk),
                                   enc=enc)


def decode_arithmetic(model, enc, text: str, context: Sequence[int], device: str = "cuda", temp: float = 1.0,
                      precision: int = 16, topk: int = 50000) -> List[int]:
    """``code_base/arithmetic.py:220`` -- the bit list the cover text decodes to."""
    return decode_arithmetic_batch(model, enc, [text], context, device=device, temp=temp, precision=precision,
                                   topk=topk)[0]


def sample_batch(model, enc, length: int, context: Optional[Sequence[int]], n: int, temperature: float = 1.0,
                 device: str = "cuda", topk: int = -1, seed: int = 0, *,
                 contexts: Optional[Sequence[Sequence[int]]] = None, lengths: Optional[Sequence[int]] = None,
                 temperatures: Optional[Sequence[float]] = None, topks: Optional[Sequence[int]] = None,
                 seeds: Optional[Sequence[int]] = None) -> List[Tuple[List[int], float, float, float]]:
    """n independent samples -> per sample ``(tokens, avg_NLL, avg_KL, avg_Hq)``.

    ``contexts``, ``lengths``, ``temperatures``, ``topks``, ``seeds`` (one entry per sample each; ``context`` is
    None with ``contexts``, and ``n == len(contexts)``) make the samples the messages of ONE slot-scheduled batch:
    sample i is ``sample(model, enc, lengths[i], contexts[i], temperatures[i], topk=topks[i], seed=seeds[i])``."""
    _ = device
    lm = _provider(model, enc)
    if any(v is not None for v in (contexts, lengths, temperatures, topks, seeds)):
        if contexts is not None and len(contexts) != int(n):
            raise ValueError(f"{len(contexts)} contexts for n = {n}")
        if lengths is None and length <= 0:
            raise ValueError("length must be positive")  # sample.py:7 asserts length > 0
        toks, stats = lm.sample_batch(
            int(n), length, list(context)[-1022:] if context is not None else None,
            contexts=[list(c)[-1022:] for c in contexts] if contexts is not None else None, lengths=lengths,
            temperatures=temperatures, topks=topks, seeds=seeds, temperature=temperature, topk=topk, seed=seed)
        return [(t, s["avg_NLL"], s["avg_KL"], s["avg_Hq"]) for t, s in zip(toks, stats)]
    if length <= 0:
        raise ValueError("length must be positive")  # sample.py:7 asserts length > 0
    toks, stats = lm.sample_batch(int(n), int(length), list(context)[-1022:], temperature=temperature, topk=topk,
                                  seed=seed)
    return [(t, s["avg_NLL"], s["avg_KL"], s["avg_Hq"]) for t, s in zip(toks, stats)]


def sample(model, enc, length: int, context: Sequence[int], temperature: float = 1.0, device: str = "cuda",
           topk: int = -1, seed: int = 0):
    """``code_base/sample.py:6`` -- returns ``(output, avg_NLL, avg_KL, avg_Hq)``."""
    return sample_batch(model, enc, length, context, 1, temperature=temperature, device=device, topk=topk,
                        seed=seed)[0]


# ---------------------------------------------------------------------------------------------------------------
# code_base/huffman_baseline.py and code_base/block_baseline.py (run_single.py's "huffman" and "bins" modes)
# ---------------------------------------------------------------------------------------------------------------
def _check_block(block_size) -> int:
    from .exceptions import ConfigurationError

    if isinstance(block_size, bool) or not isinstance(block_size, int) or not 1 <= block_size <= 8:
        raise ConfigurationError("bits_per_word / block_size must be an integer within [1, 8]")
    return block_size


def _baseline_tuple(tokens, stats):
    return tokens, stats["avg_NLL"], stats["avg_KL"], stats["words_per_bit"]


def encode_huffman_batch(model, enc, messages: Sequence[Sequence[int]], context: Optional[Sequence[int]],
                         bits_per_word: int, finish_sent: bool = False, device: str = "cuda", *,
                         contexts: Optional[Sequence[Sequence[int]]] = None, slots: Optional[int] = None
                         ) -> List[Tuple[List[int], float, float, float]]:
    """B messages (bit lists) -> per message ``(tokens, avg_NLL, avg_KL, words_per_bit)``; ``contexts`` (one per
    message, ``context`` None) makes them the messages of one slot-scheduled batch."""
    _ = device
    _check_block(bits_per_word)
    lm = _provider(model, enc)
    toks, stats = lm.encode_baseline_batch(
        [list(m) for m in messages], list(context)[-1022:] if context is not None else None,
        contexts=[list(c)[-1022:] for c in contexts] if contexts is not None else None, mode="huffman",
        block_size=bits_per_word, finish_sent=finish_sent, return_stats=True, slots=slots)
    return [_baseline_tuple(t, s) for t, s in zip(toks, stats)]


def encode_huffman(model, enc, message: Sequence[int], context: Sequence[int], bits_per_word: int,
                   finish_sent: bool = False, device: str = "cuda"):
    """``code_base/huffman_baseline.py:7`` -- returns ``(output, avg_NLL, avg_KL, words_per_bit)``."""
    return encode_huffman_batch(model, enc, [message], context, bits_per_word, finish_sent=finish_sent,
                                device=device)[0]


def decode_huffman_batch(model, enc, texts: Sequence[str], context: Optional[Sequence[int]], bits_per_word: int,
                         device: str = "cuda", *, contexts: Optional[Sequence[Sequence[int]]] = None
                         ) -> List[List[int]]:
    """B cover texts -> the bit list each decodes to, with ``decode_huffman``'s BPE repair
    (huffman_baseline.py:108-149; every emitted bit, the caller truncates)."""
    _ = device
    _check_block(bits_per_word)
    lm = _provider(model, enc)
    token_lists = [split_double_newlines(list(enc.encode(t))) for t in texts]
    return lm.decode_baseline_repair(
        token_lists, list(context)[-1022:] if context is not None else None,
        contexts=[list(c)[-1022:] for c in contexts] if contexts is not None else None, mode="huffman",
        block_size=bits_per_word, enc=enc)[0]


def decode_huffman(model, enc, text: str, context: Sequence[int], bits_per_word: int, device: str = "cuda"):
    """``code_base/huffman_baseline.py:73`` -- the bit list the cover text decodes to."""
    return decode_huffman_batch(model, enc, [text], context, bits_per_word, device=device)[0]


def get_bins(vocab_size: int, block_size: int):
    """``code_base/block_baseline.py:9`` -- ``(bin2words, words2bin)``: the reference's permutation (numpy's MT19937
    seeded with ``block_size``) drawn from a private ``RandomState``, so numpy's global generator is untouched."""
    import numpy as np

    from .coder import bins_permutation

    _check_block(block_size)
    num_bins = 2 ** block_size
    words_per_bin = vocab_size / num_bins
    order = bins_permutation(vocab_size, block_size)
    bin2words = [np.array(order[int(i * words_per_bin):int((i + 1) * words_per_bin)]) for i in range(num_bins)]
    words2bin = {}
    for j in range(num_bins):
        words2bin.update({i: j for i in bin2words[j]})
    return bin2words, words2bin


def _check_bins(lm, block_size: int, words2bin) -> None:
    """The kernels derive the bins from ``block_size`` alone; a caller's own table must be ``get_bins``'s."""
    from .coder import bins_table
    from .exceptions import ConfigurationError

    if words2bin is None:
        return
    table = bins_table(lm.vocab, block_size)
    if len(words2bin) != lm.vocab or any(int(table[int(w)]) != int(b) for w, b in words2bin.items()):
        raise ConfigurationError("words2bin is not get_bins(vocab, block_size): only the reference's bins are served")


def encode_block_batch(model, enc, messages: Sequence[Sequence[int]], context: Optional[Sequence[int]],
                       block_size: int, bin2words=None, words2bin=None, finish_sent: bool = False,
                       device: str = "cuda", *, contexts: Optional[Sequence[Sequence[int]]] = None,
                       slots: Optional[int] = None) -> List[Tuple[List[int], float, float, float]]:
    """B messages -> per message ``(tokens, avg_NLL, avg_KL, words_per_bit)`` of ``encode_block``."""
    _ = device, bin2words
    _check_block(block_size)
    lm = _provider(model, enc)
    _check_bins(lm, block_size, words2bin)
    toks, stats = lm.encode_baseline_batch(
        [list(m) for m in messages], list(context)[-1022:] if context is not None else None,
        contexts=[list(c)[-1022:] for c in contexts] if contexts is not None else None, mode="bins",
        block_size=block_size, finish_sent=finish_sent, return_stats=True, slots=slots)
    return [_baseline_tuple(t, s) for t, s in zip(toks, stats)]


def encode_block(model, enc, message: Sequence[int], context: Sequence[int], block_size: int, bin2words=None,
                 words2bin=None, finish_sent: bool = False, device: str = "cuda"):
    """``code_base/block_baseline.py:26`` -- returns ``(output, avg_NLL, avg_KL, words_per_bit)``."""
    return encode_block_batch(model, enc, [message], context, block_size, bin2words, words2bin,
                              finish_sent=finish_sent, device=device)[0]


def decode_block_batch(model, enc, texts: Sequence[str], context: Optional[Sequence[int]], block_size: int,
                       bin2words=None, words2bin=None, device: str = "cuda", *,
                       contexts: Optional[Sequence[Sequence[int]]] = None) -> List[List[int]]:
    """B cover texts -> the bit list each decodes to, with ``decode_block``'s BPE repair (block_baseline.py:140-181:
    the strict prefix test, and an unrepairable token decoded as the last bin)."""
    _ = device, bin2words
    _check_block(block_size)
    lm = _provider(model, enc)
    _check_bins(lm, block_size, words2bin)
    token_lists = [split_double_newlines(list(enc.encode(t))) for t in texts]
    return lm.decode_baseline_repair(
        token_lists, list(context)[-1022:] if context is not None else None,
        contexts=[list(c)[-1022:] for c in contexts] if contexts is not None else None, mode="bins",
        block_size=block_size, enc=enc)[0]


def decode_block(model, enc, text: str, context: Sequence[int], block_size: int, bin2words=None, words2bin=None,
                 device: str = "cuda"):
    """``code_base/block_baseline.py:99`` -- the bit list the cover text decodes to."""
    return decode_block_batch(model, enc, [text], context, block_size, bin2words, words2bin, device=device)[0]


__all__ = ["encode_arithmetic", "decode_arithmetic", "sample", "encode_arithmetic_batch", "decode_arithmetic_batch",
           "sample_batch", "split_double_newlines", "encode_huffman", "decode_huffman", "encode_huffman_batch",
           "decode_huffman_batch", "get_bins", "encode_block", "decode_block", "encode_block_batch",
           "decode_block_batch"]
