"""Token-tree speculative sampling, what needs no GPU: the refusals of tree_speculative_sampling before a model is touched."""
import pytest
import torch

from llmspeculativesampling_amd.sampling import tree_speculative_sampling

PROMPT = torch.zeros((1, 3), dtype=torch.long)


@pytest.mark.parametrize("kw,text", [(dict(branching=(8, 7)), "more than 64 nodes"), (dict(branching=(2, 9)), "level 2: 1..8 children"),
                                     (dict(branching=()), "depth 0"), (dict(rng="host"), "host-noise provider"),
                                     (dict(rng=object()), "host-noise provider"), (dict(grammar=object()), "grammar: a request option"),
                                     (dict(logprobs=True), "logprobs: a request option"), (dict(temperature=0), "temperature")],
                         ids=["65_nodes", "factor_9", "depth_0", "host_rng", "host_noise_object", "grammar", "logprobs", "temperature_0"])
def test_arguments_are_refused_before_a_model_is_touched(kw, text):
    """(8, 7) is 1 + 8 + 56 = 65 nodes.  The models are None: reaching one would raise something else."""
    with pytest.raises(ValueError, match=text):
        tree_speculative_sampling(PROMPT, None, None, 2, None, 4, **kw)
