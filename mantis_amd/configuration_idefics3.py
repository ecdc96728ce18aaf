"""Config contract of the Idefics3 path, mirroring the reference fork's `Idefics3Config`
(mantis/models/idefics3/configuration_idefics3.py:130-215): same field names and nesting (vision_config / text_config dicts,
scale_factor, image_token_id, pad_token_id), without the transformers dependency.

Field defaults are the reference's: vision 1152 wide / 3072 / 12 layers / 16 heads / 224 px / patch 32 (:81-94); text = HF LlamaConfig
defaults with rms_norm_eps 1e-5 (:204-209); image_token_id 128257, scale_factor 2, pad_token_id 128002.

Assumed, because the reference leaves it to the checkpoint's config.json and none is at hand:
  * `idefics3_8b_llama3()` takes the tower of SigLIP-so400m/14 (1152 / 4304 / 27 layers / 16 heads, as on the Idefics2 path) at the 364-px
    tile of train_idefics3.py:111 (26 x 26 patches, 169 <image> tokens per tile at scale 2) and Llama-3-8B widths with vocab 128259
    (128256 + <fake_token_around_image>, <image> = 128257, <end_of_utterance>).
  * RoPE is the default rotary embedding with theta 500000.  A text config that asks for scaled RoPE ("llama3" / linear / dynamic / yarn)
    is refused, as on the LLaVA path: it would silently change the numerics."""
from .configuration_llava import SubConfig

_VISION = dict(hidden_size=1152, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=16, num_channels=3, image_size=224,
               patch_size=32, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6, attention_dropout=0.0, initializer_range=0.02)
_TEXT = dict(model_type="llama", hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
             num_key_value_heads=None, vocab_size=32000, rope_theta=10000.0, rms_norm_eps=1e-5, hidden_act="silu", head_dim=None,
             initializer_range=0.02, tie_word_embeddings=False, attention_bias=False, mlp_bias=False)


class Idefics3Config:
    model_type = "idefics3"

    def __init__(self, use_cache=False, image_token_id=128257, tie_word_embeddings=False, vision_config=None, text_config=None,
                 scale_factor=2, pad_token_id=128002, **kwargs):
        def sub(defaults, given):
            d = dict(defaults)
            if isinstance(given, SubConfig):
                given = given.to_dict()
            d.update(given or {})
            return d
        v, t = sub(_VISION, vision_config), sub(_TEXT, text_config)
        if t["model_type"] != "llama":
            raise NotImplementedError(f"text backbone {t['model_type']!r}: the Idefics3 path is built for the Llama block")
        if t.get("attention_bias") or t.get("mlp_bias") or t.get("tie_word_embeddings") or tie_word_embeddings:
            raise NotImplementedError("attention_bias / mlp_bias / tied embeddings are not used by Idefics3-8B-Llama3")
        if t.get("num_key_value_heads") is None:
            t["num_key_value_heads"] = t["num_attention_heads"]
        if t.get("head_dim") is None:
            t["head_dim"] = t["hidden_size"] // t["num_attention_heads"]
        rp = t.get("rope_parameters") or {}
        if "rope_theta" in rp:
            t["rope_theta"] = rp["rope_theta"]
        scaling = t.get("rope_scaling")
        kinds = [rp.get("rope_type"), rp.get("type")] + ([scaling.get("rope_type"), scaling.get("type")] if scaling else [])
        if any(k not in (None, "default") for k in kinds) or (scaling and not any(kinds)):
            raise NotImplementedError(f"rope scaling {scaling or rp!r}: only the default RoPE is implemented on this path")
        if v["attention_dropout"]:
            raise NotImplementedError("attention dropout is not implemented (Idefics3 uses 0.0)")
        if isinstance(scale_factor, bool) or not isinstance(scale_factor, int) or scale_factor < 1:
            raise ValueError(f"scale_factor must be a positive integer, got {scale_factor!r}")
        t["sliding_window"] = None                  # LlamaConfig has none: full causal attention
        self.vision_config, self.text_config = SubConfig(**v), SubConfig(**t)
        self.scale_factor = scale_factor
        self.image_token_id = image_token_id
        self.pad_token_id = None if pad_token_id is None else int(pad_token_id)
        self.vocab_size = t["vocab_size"]
        self.use_cache = bool(use_cache)
        self.use_return_dict = kwargs.pop("use_return_dict", True)
        for k, val in kwargs.items():
            setattr(self, k, val)

    def to_dict(self):
        return dict(vision_config=self.vision_config.to_dict(), text_config=self.text_config.to_dict(), scale_factor=self.scale_factor,
                    image_token_id=self.image_token_id, pad_token_id=self.pad_token_id)

    def to_oracle_meta(self):
        return dict(vision=self.vision_config.to_dict(), text=self.text_config.to_dict(), image_token_id=self.image_token_id,
                    scale_factor=self.scale_factor, pad_token_id=self.pad_token_id)

    @classmethod
    def from_oracle_meta(cls, meta):
        """Build from the json blob stored in tests/golden/idefics3/weights.npz."""
        return cls(vision_config=dict(meta["vision"]), text_config=dict(meta["text"]), image_token_id=meta["image_token_id"],
                   scale_factor=meta.get("scale_factor", 2), pad_token_id=meta.get("pad_token_id"))


def idefics3_8b_llama3(**kwargs):
    """Idefics3-8B-Llama3 geometry as train_idefics3.py trains it: SigLIP-so400m/14 NaViT tower on 364-px tiles + pixel-shuffle connector
    (scale 2: 26 x 26 patches -> 169 rows of 4 * 1152) + Llama-3-8B.  See the module docstring for what is assumed."""
    return Idefics3Config(**kwargs,
        vision_config=dict(hidden_size=1152, intermediate_size=4304, num_hidden_layers=27, num_attention_heads=16, image_size=364,
                           patch_size=14),
        text_config=dict(model_type="llama", hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=128259, rope_theta=500000.0, rms_norm_eps=1e-5),
        scale_factor=2, image_token_id=128257, pad_token_id=128002)
