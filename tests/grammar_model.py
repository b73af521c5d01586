"""An oracle model whose logits carry a request's penalties, its logit edits AND its grammar mask, so that
oracle.speculative_sampling and oracle.autoregressive_sampling on wrapped models are the exact reference of the native loops'
``grammar=`` with nothing changed under oracle/.  tests/edited_model.py keeps the token prefix; the logit row at position pos
is apply_grammar(edited row, state_after(tokens[P : pos + 1])) - the state the row's own output prefix leads to, the start
state at the prompt's last row - and a row inside the prompt (j = pos + 1 - P < 0) is left unmasked."""
from edited_model import EditedModel
from llmspeculativesampling_amd.sampling.utils import apply_grammar


class GrammarModel(EditedModel):
    def __init__(self, model, prompt_len, eos_token_id, grammar, pen=(1.0, 0.0, 0.0), bias=None, allowed=None, banned=(), min_tokens=0):
        super().__init__(model, prompt_len, eos_token_id, pen, bias, allowed, banned, min_tokens)
        self.grammar = grammar

    def row(self, raw, n_hist):
        y = super().row(raw, n_hist)
        if self.grammar is None or n_hist < self.prompt_len:
            return y
        return apply_grammar(y, self.grammar, self.grammar.state_after(self.tokens[self.prompt_len:n_hist]))
