"""ClsWiseFormer on MI355X -- drop-in for the reference ``models.clswiseformer.cls_wise_former``.

Same factory (``get_cls_wise_former``), same module tree and the same 222 ``state_dict`` tensors as the reference
(cls_wise_former.py:42-278,614-780), same forward contract
``model(x[B,4,D,H,W], missing_modal) -> (prob[B,4,D,H,W], sup, edge, mid_sup, mid_edge)`` with dict keys
'01','02','04' -> prob[B,2,D,H,W] (cls_wise_former.py:585-592).  Every arithmetic op is a hand-written gfx950 kernel
from libcwf_hip.so; there is no ATen/MIOpen compute and no CPU fallback (construction works anywhere, forward needs
the built library and a GPU).

Execution: the three sub-regions share every launch between the decouplers and the cross-region coupler (grouped kernels, the
same-input decoupler convs as one conv); in training mode the supervision heads return lazy probability maps that the package's
losses consume without materialising them (cwf.functional.LazyProb).

Deliberate relaxations of reference limitations:
  * no ``fix_index.txt`` (F1): the row scatter is done on device from the top-k indices, with no host sync
    (the reference does 7 x 128 ``.item()`` round trips per forward, cls_wise_former.py:463-572);
  * batch > 1 = independent samples with the reference's B=1 semantics (F2);
  * sizes derive from the input (F3): D,H,W divisible by 16 and at least 128 semantic tokens (D*H*W >= 64^3), checked in forward;
  * the always-on stem dropout (F4) is kept by default; set ``model.Unet_list.InitConv.dropout = 0.0`` to disable.
Returned tensors are logical NC(DHW) views of channels-last (NDHWC) memory.
"""
import torch
import torch.nn as nn

from cwf import functional as CF
from cwf import coupler as CP
from cwf.kernels import backend
from .layers import HipConv, collect_convs
from .Unet_skipconnection import Unet
from .transformer import TwoClsWiseTransformerModel, FusionClsWiseTransformerModel
from .PositionalEncoding import ExtendFixedPositionalEncoding, LearnedPositionalEncoding
from .heads import SuperviseLabel, EdgeSuperviseLabel

REGIONS = ("01", "02", "04")


class ClsWiseFormer(nn.Module):
    grouped_heads = True       # the supervision heads as channel-grouped launches (False: one conv launch per region)

    def __init__(self, img_dim, patch_dim, num_channels, num_classes, embedding_dim, num_heads, num_layers, hidden_dim,
                 dropout_rate=0.0, attn_dropout_rate=0.0, conv_patch_representation=True,
                 positional_encoding_type="learned", gpu=0):
        super().__init__()
        assert embedding_dim % num_heads == 0 and img_dim % patch_dim == 0
        if positional_encoding_type not in ("fixed", "learned"):
            raise ValueError("positional_encoding_type must be 'fixed' or 'learned'")
        self.positional_encoding_type = positional_encoding_type
        self.embedding_dim, self.num_heads = embedding_dim, num_heads
        self.dropout_rate, self.attn_dropout_rate = dropout_rate, attn_dropout_rate
        self.item_feature_n, self.edge_feature_n, self.top_num = 128, 32, 128
        self.patch_size, self.edge_patch_size = (2, 2, 1), (4, 2, 2)
        tok_dim = self.item_feature_n * 2 * 2 * 1                      # 512

        # registration order reproduces the reference's state_dict order (Appendix B)
        for r in REGIONS:
            setattr(self, "e_token_" + r, nn.Parameter(torch.zeros(1, 1, tok_dim)))
            setattr(self, "s_token_" + r, nn.Parameter(torch.zeros(1, 1, tok_dim)))
        for r in REGIONS:
            nn.init.trunc_normal_(getattr(self, "e_token_" + r), std=0.02)
            nn.init.trunc_normal_(getattr(self, "s_token_" + r), std=0.02)
        for r in REGIONS:
            # "learned" (the factory's default, unused by every reference script): constructs like the reference, cannot run there or here
            setattr(self, "label_%s_position_encoding" % r, ExtendFixedPositionalEncoding(tok_dim, 1024)
                    if positional_encoding_type == "fixed" else LearnedPositionalEncoding(129, 512))
        for r in REGIONS:
            setattr(self, "transformer_" + r, TwoClsWiseTransformerModel(1, num_heads, tok_dim, dropout_rate, attn_dropout_rate))
        self.fusion_label_pos = ExtendFixedPositionalEncoding(tok_dim, 1024)
        self.fusion_transformer_1_2_4 = FusionClsWiseTransformerModel(1, num_heads, tok_dim, dropout_rate, attn_dropout_rate)
        for k in (1, 2, 4):
            setattr(self, "conv_semantic_%d" % k, HipConv(256, self.item_feature_n))
        for k in (1, 2, 4):
            setattr(self, "conv_mid_fea_%d" % k, HipConv(96, 32))
        self.Unet_list = Unet(in_channels=4, base_channels=16, num_classes=4)
        self.decoder = Decoder(embedding_dim, num_classes)
        self.supervise_label = SuperviseLabel(self.item_feature_n)
        self.edge_supervise_label = EdgeSuperviseLabel(self.edge_feature_n)
        self.mid_supervise_label = SuperviseLabel(self.item_feature_n)
        self.mid_edge_supervise_label = EdgeSuperviseLabel(self.edge_feature_n)
        self.sum_fusion = HipConv(128, 256)
        self.conv_64_to_32 = HipConv(32, 32, stride=2)

        self._packer = CF.WeightPacker()
        sem = [getattr(self, "conv_semantic_%d" % k) for k in (1, 2, 4)]
        mid = [getattr(self, "conv_mid_fea_%d" % k) for k in (1, 2, 4)]
        collect_convs(self, self._packer, skip=sem + mid)
        # the three same-input decoupler convs of each kind run as ONE conv (256 -> 3 x 128, 96 -> 3 x 32); parameters stay separate
        self._sem_spec = CF.FusedConvSpec(sem[0].spec.op, 256, self.item_feature_n)
        self._mid_spec = CF.FusedConvSpec(mid[0].spec.op, 96, 32)
        self._packer.add_fused(self._sem_spec, [m.weight for m in sem], [m.bias for m in sem])
        self._packer.add_fused(self._mid_spec, [m.weight for m in mid], [m.bias for m in mid])
        # test / analysis hooks (not part of the reference interface)
        self.forced_index = None      # dict name -> int tensor [B,k]: teacher-forced top-k selections
        self.collect_aux = False
        self.aux = {}
        self.phase_callback = None    # set by cwf.trainer.Trainer: called with k when backward has passed cut point k (grad_phases)

    def grad_phases(self):
        """Parameters grouped by WHEN their gradients are final during backward (the order of the Trainer's flat gradient buffer):
        phase 0 the decoder (backward starts there), phase 1 everything between the decoder and the encoder (heads, both couplers,
        the decoupler convs, sum_fusion), phase 2 the encoder and conv_64_to_32.  The cut points are the gradients of the decoder's
        input (phase 0 done) and of the decouplers' inputs x23 / x4 (phase 1 done); forward registers hooks there when
        `phase_callback` is set, so that a phase's slice can be reduced / all-reduced while backward continues."""
        dec = list(self.decoder.parameters())
        enc = list(self.Unet_list.parameters()) + list(self.conv_64_to_32.parameters())
        # the fused decoupler layers reduce into ONE slice each: keep their three weights (and three biases) adjacent
        fused = []
        for name in ("conv_semantic_%d", "conv_mid_fea_%d"):
            mods = [getattr(self, name % k) for k in (1, 2, 4)]
            fused += [m.weight for m in mods] + [m.bias for m in mods]
        skip = {id(p) for p in dec + enc + fused}
        mid = fused + [p for p in self.parameters() if id(p) not in skip]
        return [dec, mid, enc]

    def _cut(self, t, k, need=1):
        """register the phase-k cut on tensor t (phase complete after `need` such cuts have fired)"""
        cb = self.phase_callback
        if cb is None or not torch.is_grad_enabled() or not t.requires_grad:
            return
        state = self._cut_state.setdefault(k, [0, need])

        def hook(g):
            state[0] += 1
            if state[0] == state[1]:
                cb(k)
            return None
        t.register_hook(hook)

    # ------------------------------------------------------------------------------------------------
    def _coupler_cfg(self, tr, names, groups=1):
        """Dropout rates are read from the module tree at call time (tests zero them; the reference's values are 0.1)."""
        pre = tr.cross_attention_list[0].fn
        ff = tr.cross_ffn_list[0].fn.fn
        return CP.CouplerConfig(self.num_heads, self.top_num, self.training, self.dropout_rate, pre.fn.dropout_rate, pre.dropout_rate,
                                ff.dropout_rate, forced=self.forced_index, names=names, groups=groups)

    def _heads3(self, heads, feats_all):
        """the three sub-regions' supervision heads on the channel groups of one tensor (zero-copy slices)"""
        if self.grouped_heads:
            return heads.heads3(feats_all)               # both conv stages as one channel-grouped launch each way
        parts = CP.split_channels3(feats_all)
        return {r: heads.head(k, p) for r, k, p in zip(REGIONS, (1, 2, 4), parts)}

    def encode(self, x, missing_modal=None):
        x1, x2, x3, x4 = self.Unet_list(x)
        x2d, _, x2 = self.conv_64_to_32(x2, carry=True)           # :284 (x2 goes on to the decoder through the carry alias)
        x23 = CF.cat_channels(x2d, x3)
        self._cut(x23, 1, need=2)
        self._cut(x4, 1, need=2)
        G = len(REGIONS)
        # edge decoupler (:284-296) and Anatomy-induced Region Decoupler (:314-324): the three same-input convs of each as one launch
        f, s = CF.fused_conv3(x23, [getattr(self, "conv_mid_fea_%d" % k) for k in (1, 2, 4)], self._mid_spec)
        ef = CF.norm_act_add(f, s, 0.01)                           # [B,32^3,3*32]
        f, s = CF.fused_conv3(x4, [getattr(self, "conv_semantic_%d" % k) for k in (1, 2, 4)], self._sem_spec)
        sf = CF.norm_act_add(f, s, 0.01)                           # [B,16^3,3*128]
        mid_sup = self._heads3(self.mid_supervise_label, sf)       # :332
        mid_edge = self._heads3(self.mid_edge_supervise_label, ef)  # :333
        sem_size, edge_size = tuple(sf.shape[1:4]), tuple(ef.shape[1:4])
        E = CP.window_to_tokens_g(ef, G, self.edge_patch_size)     # [3,B,Ne,512]  :341
        S = CP.window_to_tokens_g(sf, G, self.patch_size)          # [3,B,Ns,512]  :342
        # selection (:345-376) -> Edge-supported Intra-region Coupler (:379) -> scatter + gate (:463-485), all three regions per launch
        names = [(r + "_edge", r + "_sem_supp", r + "_sem", r + "_edge_supp") for r in REGIONS]
        trs = [getattr(self, "transformer_" + r) for r in REGIONS]
        cfg = self._coupler_cfg(trs[0], names, groups=G)
        flat = [getattr(self, "e_token_" + r) for r in REGIONS] + [getattr(self, "s_token_" + r) for r in REGIONS]
        for tr in trs:
            flat += list(CP.transformer_params(tr))
        out = CP.RegionCouplerFn.apply(cfg, E, S, *flat)
        gated_e, gated_s, scat_s, sem_tok = out[:4]
        if self.collect_aux:
            b = x.shape[0]
            for j, idx in enumerate(out[4:]):
                for g in range(G):
                    self.aux[names[g][j]] = idx[g * b:(g + 1) * b]
        sup_edge = CP.tokens_to_window_g(gated_e, edge_size, self.edge_feature_n, self.edge_patch_size)
        sup_sem = CP.tokens_to_window_g(gated_s, sem_size, self.item_feature_n, self.patch_size)
        sup = self._heads3(self.supervise_label, sup_sem)          # :545
        edge = self._heads3(self.edge_supervise_label, sup_edge)   # :546

        # Mutual Cross-region Coupler (:549-579): post-scatter UN-gated semantic tokens are fused
        f_tok = CP.sum_groups3(sem_tok)
        f_feat = CP.sum_groups3(scat_s)
        tr = self.fusion_transformer_1_2_4
        fused, f_idx = CP.FusionCouplerFn.apply(self._coupler_cfg(tr, [("fusion",)]), f_feat, f_tok, *CP.transformer_params(tr))
        if self.collect_aux:
            self.aux["fusion"] = f_idx
        xb = CF.tokens_to_window(fused, sem_size, self.item_feature_n, self.patch_size)
        xb, _ = self.sum_fusion(xb)                                   # :582
        self._cut(xb, 0)
        if self.collect_aux:
            self.aux["bottleneck"] = xb
        return x1, x2, x3, xb, sup, edge, mid_sup, mid_edge

    def forward(self, x, missing_modal=None):
        backend()                                                     # raises if the HIP library / GPU is missing
        if self.positional_encoding_type != "fixed":
            raise RuntimeError("_pe_type='learned': the reference builds LearnedPositionalEncoding(129, 512), a [1,512,129] parameter that "
                               "cannot be added to the [B,128,512] token rows (cls_wise_former.py:87-90,348) -- its forward raises too; "
                               "every reference script passes _pe_type='fixed' (train_no_amp.py:130)")
        if x.dim() != 5 or x.shape[1] != 4:
            raise ValueError("expected x of shape [B,4,D,H,W], got %s" % (tuple(x.shape),))
        _, _, d, h, w = x.shape
        if d % 16 or h % 16 or w % 16:
            raise ValueError("D, H, W must be multiples of 16 (got %d,%d,%d)" % (d, h, w))
        if (d // 16) * (h // 16) * (w // 8) < self.top_num:
            # every selection takes exactly top_num rows, so that the four sequences of a region have one length and the coupler
            # runs as batches of sequence pairs (the reference's own sizes give 1024 / 2048 tokens)
            raise ValueError("the patch must yield at least %d semantic tokens: D*H*W >= %d (got %dx%dx%d)"
                             % (self.top_num, self.top_num * 2048, d, h, w))
        self.aux = {}
        self._cut_state = {}
        # every conv output / block tail of this model has ONE gradient consumer: a backward pass may hand on a bf16 gradient image alone
        # (declared for this forward pass only; other graphs in the process keep their fp32 gradients)
        with CF.single_consumer_graph():
            backend().begin_step(x.device)
            self._packer.refresh()
            xc = x.to(torch.float32).permute(0, 2, 3, 4, 1).contiguous()  # NDHWC
            x1, x2, x3, xb, sup, edge, mid_sup, mid_edge = self.encode(xc, missing_modal)
            prob = self.decoder(x1, x2, x3, None, xb, aux=self.aux if self.collect_aux else None)
        return prob, sup, edge, mid_sup, mid_edge


class EnBlock2(nn.Module):
    """conv -> IN -> LeakyReLU -> conv -> IN -> LeakyReLU -> + x  (cls_wise_former.py:691-713; DeBlock :732-754 is identical)"""

    def __init__(self, in_channels):
        super().__init__()
        self.conv1 = HipConv(in_channels, in_channels)
        self.conv2 = HipConv(in_channels, in_channels)

    def forward(self, x, emit16=False):
        h, hs, xc = self.conv1(x, want_stats=True, carry=True)        # the residual's gradient is folded into conv1's dgrad epilogue
        g, gs = self.conv2(h, in_norm=hs, slope=0.01, want_stats=True)
        # emit16: the next block's conv1 reads this output without a prologue -- its weight gradient takes the bf16 image written here
        return CF.norm_act_add(g, gs, 0.01, residual=xc, emit16=emit16)


class DeBlock(EnBlock2):
    pass


class DeUp_Cat(nn.Module):
    """1x1 conv -> ConvTranspose k2 s2 -> concat(prev, y) -> 1x1 conv  (cls_wise_former.py:716-729)"""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = HipConv(in_channels, out_channels, k=1)
        self.conv2 = HipConv(out_channels, out_channels, transposed=True)
        self.conv3 = HipConv(out_channels * 2, out_channels, k=1)

    def forward(self, x, prev):
        t, _ = self.conv1(x)
        buf = getattr(prev, "_cwf_catbuf", None)              # the encoder wrote the skip tensor into its concatenation buffer already
        if buf is None or buf.shape[-1] != prev.shape[-1] + self.conv2.spec.cout or buf.data_ptr() != prev.data_ptr():
            buf = CF.cat_buffer(prev, self.conv2.spec.cout)
        hi = buf[..., prev.shape[-1]:] if buf.data_ptr() != prev.data_ptr() else CF.alias_channels(buf, prev.shape[-1], buf.shape[-1])
        u, _ = self.conv2(t, out=hi)                              # the transposed conv writes its half of the concatenation in place
        y, _ = self.conv3(CF.cat_into(prev, u, buf), emit16=True)    # (its output is the next block's un-normalised conv input)
        return y


class Decoder(nn.Module):
    def __init__(self, embedding_dim, num_classes):
        super().__init__()
        e = embedding_dim
        self.down_channel = HipConv(e, e // 2, k=1)
        self.Enblock8_1 = EnBlock2(e // 2)
        self.Enblock8_2 = EnBlock2(e // 2)
        self.DeUp4 = DeUp_Cat(e // 2, e // 4)
        self.DeBlock4 = DeBlock(e // 4)
        self.DeBlock4_1 = DeBlock(e // 4)
        self.DeUp3 = DeUp_Cat(e // 4, e // 8)
        self.DeBlock3 = DeBlock(e // 8)
        self.DeBlock3_1 = DeBlock(e // 8)
        self.DeUp2 = DeUp_Cat(e // 8, e // 16)
        self.DeBlock2 = DeBlock(e // 16)
        self.DeBlock2_1 = DeBlock(e // 16)
        self.endconv = HipConv(e // 16, num_classes, k=1)

    def forward(self, x1_1, x2_1, x3_1, x4_1, x, aux=None):
        x8, _ = self.down_channel(x)
        # emit16: the next block's conv1 takes this block's output without a prologue (bf16 image for its weight gradient)
        x8 = self.Enblock8_2(self.Enblock8_1(x8, emit16=True))
        y4 = self.DeBlock4_1(self.DeBlock4(self.DeUp4(x8, x3_1), emit16=True))
        y3 = self.DeBlock3_1(self.DeBlock3(self.DeUp3(y4, x2_1), emit16=True))
        y2 = self.DeBlock2_1(self.DeBlock2(self.DeUp2(y3, x1_1), emit16=True))
        logits, _ = self.endconv(y2)
        if aux is not None:
            aux["logits"] = logits.permute(0, 4, 1, 2, 3)
        return CF.channel_softmax(logits).permute(0, 4, 1, 2, 3)      # cls_wise_former.py:662-664


def get_cls_wise_former(dataset="brats", _conv_repr=True, _pe_type="learned", gpu=0):
    """Factory with the reference signature (cls_wise_former.py:757-780); ``dataset``, ``_conv_repr`` and ``gpu`` do
    not change behaviour there either.  Every reference caller passes ``_pe_type='fixed'``."""
    if dataset.lower() != "brats":
        raise ValueError("unknown dataset %r" % dataset)
    return ClsWiseFormer(128, 16, 4, 4, embedding_dim=256, num_heads=8, num_layers=1, hidden_dim=2048,
                         dropout_rate=0.1, attn_dropout_rate=0.1, conv_patch_representation=_conv_repr,
                         positional_encoding_type=_pe_type, gpu=gpu)
