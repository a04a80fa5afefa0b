"""TEST INFRASTRUCTURE (never imported by the product): the paged KV cache restated in plain torch.

  * page maps: which page holds entry e of row b's table -- identity, reversed, interleaved across rows, a seeded permutation.  Page 0,
    the scrap page, is never in a map;
  * scatter / gather between a contiguous cache [B, cap, 2, H, 128] and a page pool under a map: `gather(scatter(c)) == c`;
  * PagedOracleOps: the two methods of the optional group "kv_paged" as gather + the contiguous oracle op, for the CPU tests of the
    scheduler and the model plumbing.
"""
import torch

from evo_amd.sh.cache import PagedKV
from test_ragged_prefill_host import RaggedOracleOps

PAGE_MAPS = ("identity", "reversed", "interleaved", "random")


def page_map(kind, B, width, seed=0, spare=0):
    """[B, width] int64: the page id of entry e of row b.  Ids are distinct and lie in 1 .. B * width + spare (`spare` pages, and page 0,
    are owned by no row)."""
    n = B * width
    if kind == "identity":
        ids = torch.arange(n).view(B, width)
    elif kind == "reversed":
        ids = torch.arange(n - 1, -1, -1).view(B, width)
    elif kind == "interleaved":                                       # neighbouring entries of a row are B pages apart
        ids = (torch.arange(width)[None, :] * B + torch.arange(B)[:, None])
    elif kind == "random":
        ids = torch.randperm(n + spare, generator=torch.Generator().manual_seed(seed))[:n].view(B, width)
        return ids + 1
    else:
        raise ValueError(kind)
    return ids + 1 + spare // 2


def n_pages_of(B, width, spare=0):
    return 1 + B * width + spare


def scatter(cache, pmap, page_tokens, n_pages, lengths=None, out=None):
    """cache [B, cap, 2, H, hd] -> pages [n_pages, page_tokens, 2, H, hd] under pmap [B, width] (width * page_tokens >= the tokens
    written).  lengths: only tokens [0, lengths[b]) of row b are written.  out: an existing pool (e.g. pre-filled with poison); a fresh
    pool is zeros."""
    B, cap = cache.shape[:2]
    pages = out if out is not None else torch.zeros(n_pages, page_tokens, *cache.shape[2:], dtype=cache.dtype, device=cache.device)
    pm = pmap.to(cache.device)
    for b in range(B):
        n = cap if lengths is None else int(lengths[b])
        t = torch.arange(n, device=cache.device)
        pages[pm[b, t // page_tokens], t % page_tokens] = cache[b, :n]
    return pages


def gather(pages, table, n_tokens):
    """[B, n_tokens, 2, H, hd]: tokens 0 .. n_tokens - 1 of every table row."""
    pt = pages.shape[1]
    t = torch.arange(n_tokens, device=pages.device)
    return pages[table.long()[:, t // pt], (t % pt)[None, :]]


def table_of(pmap, width=None, device="cpu"):
    """The int32 device table of a map, padded with zeros (the scrap page) to `width` entries."""
    B, w = pmap.shape
    t = torch.zeros(B, w if width is None else width, dtype=torch.int32)
    t[:, :w] = pmap.to(torch.int32)
    return t.to(device)


class PagedOps:
    """The optional group "kv_paged" on an oracle backend (mixed in in front of it): gather the row's tokens, then the contiguous op."""

    def rope_append_decode_paged(self, qkv, kv, pos, inv_freq, scaling, q_scale=1.0):
        assert q_scale == 1.0 and isinstance(kv, PagedKV)
        self.paged_calls["append"] += 1
        B, _, _, H, hd = qkv.shape
        t = pos.to(torch.float32)
        if scaling != 1.0:
            t = t / scaling
        freqs = torch.outer(t, inv_freq)                              # (StripedHyena._rotary_dyn, the table of the contiguous path)
        self.rope_(qkv.view(1, B, 3, H, hd), torch.cos(freqs).to(torch.bfloat16).float().contiguous(),
                   torch.sin(freqs).to(torch.bfloat16).float().contiguous())
        pt = kv.page_tokens
        pg = kv.table[torch.arange(B), (pos // pt)].long()
        kv.pages[pg, pos % pt] = qkv[:, 0, 1:3]

    def attention_decode_paged(self, q, kv, pos, n_splits=None, prescaled=False):
        assert not prescaled and isinstance(kv, PagedKV) and pos.numel() == q.shape[0]
        self.paged_calls["decode"] += 1
        c = gather(kv.pages, kv.table[:q.shape[0]], int(pos.max()) + 1)
        return self.attention_decode(q, c[:, :, 0], c[:, :, 1], pos=pos)


class PagedOracleOps(PagedOps, RaggedOracleOps):
    def __init__(self, act=torch.float64):
        super().__init__(act)
        self.paged_calls = {"append": 0, "decode": 0}
