"""CPU: the tensor tokens of gslm._lib (tensor_token / token_matches / tokens_match), which key everything the Python
layer derives from a tensor's contents and keeps: LossEvaluator's depth orders (xyz), ViewRaster.active_params' block
(four leaves) and LMProblem.rhs_is_mine.

A token matches only the same tensor object at the same version.  It holds the object, so while the token lives the
storage cannot be handed to another tensor -- which is what lets the address stay out of the key."""
import gc

import torch


def _tok():
    from gslm import _lib
    return _lib.tensor_token, _lib.token_matches, _lib.tokens_match


def test_matches_the_same_tensor_at_the_same_version():
    tensor_token, token_matches, _ = _tok()
    t = torch.arange(6.0)
    tok = tensor_token(t)
    assert token_matches(tok, t)
    assert token_matches(tok, t)  # (matching changes nothing)
    assert tok[0] is t  # the token holds the tensor
    assert not token_matches(None, t)
    p = torch.nn.Parameter(torch.zeros(3))
    assert token_matches(tensor_token(p), p)


def test_misses_after_an_in_place_write():
    tensor_token, token_matches, _ = _tok()
    t = torch.zeros(4)
    for write in (lambda: t.add_(1.0), lambda: t.zero_(), lambda: t[1:3].fill_(2.0),
                  lambda: t.copy_(torch.ones(4)), lambda: t.view(2, 2).mul_(3.0)):
        tok = tensor_token(t)
        write()
        assert not token_matches(tok, t)
        assert token_matches(tensor_token(t), t)
    p = torch.nn.Parameter(torch.zeros(3))
    tok = tensor_token(p)
    with torch.no_grad():
        p.add_(1.0)
    assert not token_matches(tok, p)


def test_misses_after_increment_version():
    """The bump a Python-layer call gives a tensor it wrote through a raw pointer (FusedAdam.step)."""
    tensor_token, token_matches, _ = _tok()
    t = torch.zeros(4)
    tok = tensor_token(t)
    v = t._version
    torch.autograd.graph.increment_version(t)
    assert t._version == v + 1
    assert not token_matches(tok, t)
    p = torch.nn.Parameter(torch.zeros(3))
    tok = tensor_token(p)
    torch.autograd.graph.increment_version(p)
    assert not token_matches(tok, p)


def test_misses_for_another_tensor_object():
    tensor_token, token_matches, _ = _tok()
    t = torch.zeros(4)
    tok = tensor_token(t)
    d = t.detach()
    # the alias an address-and-version key cannot tell from t
    assert d is not t and d.data_ptr() == t.data_ptr() and d._version == t._version
    assert not token_matches(tok, d)
    assert not token_matches(tok, t.view(4))
    assert not token_matches(tok, t.clone())
    assert not token_matches(tok, torch.zeros(4))
    assert token_matches(tok, t)


def test_the_token_keeps_the_storage_from_being_reused():
    """A dropped tensor's token still holds it: a tensor made afterwards is another object (and on an allocator that
    reuses freed blocks, cannot be at its address)."""
    tensor_token, token_matches, _ = _tok()
    t = torch.zeros(1000)
    addr = t.data_ptr()
    tok = tensor_token(t)
    del t
    gc.collect()
    fresh = [torch.zeros(1000) for _ in range(8)]
    assert all(f.data_ptr() != addr for f in fresh)
    assert not any(token_matches(tok, f) for f in fresh)
    assert tok[0].data_ptr() == addr and token_matches(tok, tok[0])


def test_a_tuple_of_tokens_misses_when_any_leaf_changed():
    tensor_token, _, tokens_match = _tok()
    leaves = [torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(5, 1)]
    toks = tuple(tensor_token(t) for t in leaves)
    assert tokens_match(toks, leaves)
    assert not tokens_match(None, leaves)
    assert not tokens_match(toks, leaves[:3]) and not tokens_match(toks[:3], leaves)
    for j in range(len(leaves)):
        toks = tuple(tensor_token(t) for t in leaves)
        leaves[j].add_(1.0)  # written in place
        assert not tokens_match(toks, leaves), j
        toks = tuple(tensor_token(t) for t in leaves)
        assert tokens_match(toks, leaves)
        old, leaves[j] = leaves[j], leaves[j].detach()  # replaced by an alias at the same address and version
        assert not tokens_match(toks, leaves), j
        leaves[j] = old
        assert tokens_match(toks, leaves)
    # the same tensors in another order are other leaves
    toks = tuple(tensor_token(t) for t in leaves)
    assert not tokens_match(toks, [leaves[1], leaves[0]] + leaves[2:])
