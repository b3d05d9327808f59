"""openai/CLIP's `CLIP.encode_text` (clip/model.py) restated on torch over an OpenAI-layout weight dict, in the dtype of the weights: the
reference of the text tower's checks (text_checks.py).  float64 weights give the fp64 truth, float32 weights the fp32 evaluation whose own gap
to fp64 the kernel's gate is taken from.  test_text_ref_vs_transformers pins it against transformers.CLIPTextModelWithProjection in fp64."""
import torch
import torch.nn.functional as F


def encode_text(w, tokens, cfg):
    """w: token_embedding.weight, positional_embedding, transformer.resblocks.N.*, ln_final.*, text_projection; tokens: int [n, ctx]
    -> [n, output_dim]: ln_final of the row at tokens.argmax(-1) (the EOT, the largest id) times text_projection"""
    tokens = tokens.long()
    n, ctx = tokens.shape
    D, heads = cfg['width'], cfg['heads']
    dt = w['token_embedding.weight'].dtype
    x = w['token_embedding.weight'][tokens] + w['positional_embedding'][:ctx]
    mask = torch.full((ctx, ctx), float('-inf'), dtype=dt).triu_(1)              # build_attention_mask
    for i in range(cfg['layers']):
        p = 'transformer.resblocks.%d.' % i
        h = F.layer_norm(x, (D,), w[p + 'ln_1.weight'], w[p + 'ln_1.bias'], 1e-5)
        qkv = h @ w[p + 'attn.in_proj_weight'].t() + w[p + 'attn.in_proj_bias']
        q, k, v = (t.reshape(n, ctx, heads, D // heads).transpose(1, 2) for t in qkv.split(D, dim=-1))
        a = torch.softmax(q @ k.mT * (D // heads) ** -0.5 + mask, dim=-1) @ v
        x = x + a.transpose(1, 2).reshape(n, ctx, D) @ w[p + 'attn.out_proj.weight'].t() + w[p + 'attn.out_proj.bias']
        h = F.layer_norm(x, (D,), w[p + 'ln_2.weight'], w[p + 'ln_2.bias'], 1e-5)
        u = h @ w[p + 'mlp.c_fc.weight'].t() + w[p + 'mlp.c_fc.bias']
        x = x + (u * torch.sigmoid(1.702 * u)) @ w[p + 'mlp.c_proj.weight'].t() + w[p + 'mlp.c_proj.bias']
    x = F.layer_norm(x, (D,), w['ln_final.weight'], w['ln_final.bias'], 1e-5)
    return x[torch.arange(n), tokens.argmax(dim=-1)] @ w['text_projection']


def to_transformers_state(w, cfg):
    """the same weights under transformers.CLIPTextModelWithProjection's names (in_proj split into q / k / v, text_projection transposed)"""
    D = cfg['width']
    sd = {'text_model.embeddings.token_embedding.weight': w['token_embedding.weight'],
          'text_model.embeddings.position_embedding.weight': w['positional_embedding'],
          'text_model.final_layer_norm.weight': w['ln_final.weight'], 'text_model.final_layer_norm.bias': w['ln_final.bias'],
          'text_projection.weight': w['text_projection'].t().contiguous()}
    for i in range(cfg['layers']):
        p, h = 'transformer.resblocks.%d.' % i, 'text_model.encoder.layers.%d.' % i
        for j, n in enumerate(('q_proj', 'k_proj', 'v_proj')):
            sd[h + 'self_attn.%s.weight' % n] = w[p + 'attn.in_proj_weight'][j * D:(j + 1) * D]
            sd[h + 'self_attn.%s.bias' % n] = w[p + 'attn.in_proj_bias'][j * D:(j + 1) * D]
        for a, b in (('attn.out_proj', 'self_attn.out_proj'), ('ln_1', 'layer_norm1'), ('ln_2', 'layer_norm2'), ('mlp.c_fc', 'mlp.fc1'),
                     ('mlp.c_proj', 'mlp.fc2')):
            sd[h + b + '.weight'] = w[p + a + '.weight']
            sd[h + b + '.bias'] = w[p + a + '.bias']
    return sd
