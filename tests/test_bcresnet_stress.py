"""The BcResNet head's stressed models and clips (tests/test_gpu_bcresnet_stress.py runs them on the HIP path), and a numpy emulator of its
two-term binary16 arithmetic: the front kernel under its plan-time scales (features clamped to +-8192, one f16_wscale for the init conv),
and each block's two products (dual_x3 AT = 3, bc_chain) with every pixel row of d and of xs under its own power of two (the row's largest
element into [2^14, 2^15): eb = clamp(biased exponent, 16, 254), scale 2^(141 - eb); one scale per 32-pixel group of a clip where the last
block averages in the same launch) and one f16_wscale per weight tensor.  Every block's shortcut is a 1x1 conv + BatchNorm, not an
identity, so a per-channel power of two on a block's output IS undone in the next block's pointwise and shortcut.0 columns - the same
function, bit for bit in float32 - and an element 2^g below its row's (its tensor's) largest keeps min(22, 38 - g) bits.

Cases (ReLU): l0 - init_conv.1's weight and bias [c] x 2^g, block1's pointwise and shortcut.0 columns c / 2^g; l1, l2 - block i's bn1 AND
shortcut.1 [c] x 2^g, block i + 1's columns / 2^g; l3 - block3's two BatchNorms against fc.weight[:, c] (float32 tail: the control);
dw1 .. dw3 - block i's depthwise[c] x 2^g, its pointwise[:, c] / 2^g (legal under every activation); l01 - l0 on channel 3 with l1 on
channel 5.  g in +-{8, 12, 16, 20, 24}.  GELU / SiLU heads: the BN-link edits are no longer the same function; they are models like any
other, judged against float64 on their own weights (UNBALANCED).

The fix this file came with: balance() (balance_channel_gains, extended to this head: the init conv's BatchNorm, each block's two
BatchNorms as one channel, each depthwise against its pointwise) brings every ReLU case - and every dw case under any activation - back to
the plain weights' arithmetic, and what cannot be balanced is held by plan()'s per-block guard (f16_pixel_rows_ok, plan_host.h), which
sends a block to the three-term bf16 form (emulated as exact).

The emulator's table at (32, 40) - max |logit - float64| / max(1, |logit|max) on 33 clips of synth_features(seed 9); "before": the weights
as given, every block on two terms; "after": balanced, then guarded; forms as block1/block2/block3, 2 = two binary16 terms, 3 = three
bf16 terms.  table() prints it for both shapes; (70, 64) tells the same.  The float32 oracle's own error is on every row:

relu                32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
gelu                32x40  f32 1.6e-06 | before 2/2/2 3.3e-07 | after 2/2/2 3.3e-07
silu                32x40  f32 1.9e-06 | before 2/2/2 2.7e-07 | after 2/2/2 2.7e-07
l0-2^8              32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l1-2^8              32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l2-2^8              32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l3-2^8              32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw1-2^8             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw2-2^8             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw3-2^8             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l01-2^8             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l0-2^-8             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l1-2^-8             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l2-2^-8             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l3-2^-8             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw1-2^-8            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw2-2^-8            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw3-2^-8            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l01-2^-8            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l0-2^12             32x40  f32 1.1e-06 | before 2/2/2 2.3e-07 | after 2/2/2 2.4e-07
l1-2^12             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l2-2^12             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l3-2^12             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw1-2^12            32x40  f32 1.1e-06 | before 2/2/2 2.3e-07 | after 2/2/2 2.4e-07
dw2-2^12            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw3-2^12            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l01-2^12            32x40  f32 1.1e-06 | before 2/2/2 2.3e-07 | after 2/2/2 2.4e-07
l0-2^-12            32x40  f32 1.1e-06 | before 2/2/2 2.3e-07 | after 2/2/2 2.4e-07
l1-2^-12            32x40  f32 1.1e-06 | before 2/2/2 2.3e-07 | after 2/2/2 2.4e-07
l2-2^-12            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l3-2^-12            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw1-2^-12           32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw2-2^-12           32x40  f32 1.1e-06 | before 2/2/2 2.3e-07 | after 2/2/2 2.4e-07
dw3-2^-12           32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
l01-2^-12           32x40  f32 1.1e-06 | before 2/2/2 2.2e-07 | after 2/2/2 2.4e-07
l0-2^16             32x40  f32 1.1e-06 | before 2/2/2 2.7e-07 | after 2/2/2 2.4e-07
l1-2^16             32x40  f32 1.1e-06 | before 2/2/2 2.5e-07 | after 2/2/2 2.4e-07
l2-2^16             32x40  f32 1.1e-06 | before 2/2/2 2.7e-07 | after 2/2/2 2.4e-07
l3-2^16             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw1-2^16            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw2-2^16            32x40  f32 1.1e-06 | before 2/2/2 2.3e-07 | after 2/2/2 2.4e-07
dw3-2^16            32x40  f32 1.1e-06 | before 2/2/2 2.6e-07 | after 2/2/2 2.4e-07
l01-2^16            32x40  f32 1.1e-06 | before 2/2/2 2.8e-07 | after 2/2/2 2.4e-07
l0-2^-16            32x40  f32 1.1e-06 | before 2/2/2 1.9e-07 | after 2/2/2 2.4e-07
l1-2^-16            32x40  f32 1.1e-06 | before 2/2/2 2.1e-07 | after 2/2/2 2.4e-07
l2-2^-16            32x40  f32 1.1e-06 | before 2/2/2 1.9e-07 | after 2/2/2 2.4e-07
l3-2^-16            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw1-2^-16           32x40  f32 1.1e-06 | before 2/2/2 2.2e-07 | after 2/2/2 2.4e-07
dw2-2^-16           32x40  f32 1.1e-06 | before 2/2/2 2.0e-07 | after 2/2/2 2.4e-07
dw3-2^-16           32x40  f32 1.1e-06 | before 2/2/2 2.2e-07 | after 2/2/2 2.4e-07
l01-2^-16           32x40  f32 1.1e-06 | before 2/2/2 2.7e-07 | after 2/2/2 2.4e-07
l0-2^20             32x40  f32 1.1e-06 | before 2/2/2 7.9e-07 | after 2/2/2 2.4e-07
l1-2^20             32x40  f32 1.1e-06 | before 2/2/2 6.5e-07 | after 2/2/2 2.4e-07
l2-2^20             32x40  f32 1.1e-06 | before 2/2/2 2.2e-06 | after 2/2/2 2.4e-07
l3-2^20             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw1-2^20            32x40  f32 1.1e-06 | before 2/2/2 4.0e-07 | after 2/2/2 2.4e-07
dw2-2^20            32x40  f32 1.1e-06 | before 2/2/2 4.0e-07 | after 2/2/2 2.4e-07
dw3-2^20            32x40  f32 1.1e-06 | before 2/2/2 2.2e-06 | after 2/2/2 2.4e-07
l01-2^20            32x40  f32 1.1e-06 | before 2/2/2 1.7e-06 | after 2/2/2 2.4e-07
l0-2^-20            32x40  f32 1.1e-06 | before 2/2/2 2.7e-06 | after 2/2/2 2.4e-07
l1-2^-20            32x40  f32 1.1e-06 | before 2/2/2 2.1e-06 | after 2/2/2 2.4e-07
l2-2^-20            32x40  f32 1.1e-06 | before 2/2/2 4.7e-06 | after 2/2/2 2.4e-07
l3-2^-20            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw1-2^-20           32x40  f32 1.1e-06 | before 2/2/2 1.3e-06 | after 2/2/2 2.4e-07
dw2-2^-20           32x40  f32 1.1e-06 | before 2/2/2 9.6e-07 | after 2/2/2 2.4e-07
dw3-2^-20           32x40  f32 1.1e-06 | before 2/2/2 2.1e-06 | after 2/2/2 2.4e-07
l01-2^-20           32x40  f32 1.1e-06 | before 2/2/2 4.3e-06 | after 2/2/2 2.4e-07
l0-2^24             32x40  f32 1.1e-06 | before 2/2/2 9.7e-06 | after 2/2/2 2.4e-07
l1-2^24             32x40  f32 1.1e-06 | before 2/2/2 6.0e-06 | after 2/2/2 2.4e-07
l2-2^24             32x40  f32 1.1e-06 | before 2/2/2 2.3e-05 | after 2/2/2 2.4e-07
l3-2^24             32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw1-2^24            32x40  f32 1.1e-06 | before 2/2/2 6.7e-06 | after 2/2/2 2.4e-07
dw2-2^24            32x40  f32 1.1e-06 | before 2/2/2 3.4e-06 | after 2/2/2 2.4e-07
dw3-2^24            32x40  f32 1.1e-06 | before 2/2/2 1.8e-05 | after 2/2/2 2.4e-07
l01-2^24            32x40  f32 1.1e-06 | before 2/2/2 2.1e-05 | after 2/2/2 2.4e-07
l0-2^-24            32x40  f32 1.1e-06 | before 2/2/2 4.1e-05 | after 2/2/2 2.4e-07
l1-2^-24            32x40  f32 1.1e-06 | before 2/2/2 6.9e-05 | after 2/2/2 2.4e-07
l2-2^-24            32x40  f32 1.1e-06 | before 2/2/2 1.9e-05 | after 2/2/2 2.4e-07
l3-2^-24            32x40  f32 1.1e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
dw1-2^-24           32x40  f32 1.1e-06 | before 2/2/2 2.6e-05 | after 2/2/2 2.4e-07
dw2-2^-24           32x40  f32 1.1e-06 | before 2/2/2 6.9e-05 | after 2/2/2 2.4e-07
dw3-2^-24           32x40  f32 1.1e-06 | before 2/2/2 1.4e-05 | after 2/2/2 2.4e-07
l01-2^-24           32x40  f32 1.1e-06 | before 2/2/2 9.5e-05 | after 2/2/2 2.4e-07
gelu-dw1-2^-24      32x40  f32 1.6e-06 | before 2/2/2 2.0e-05 | after 2/2/2 3.3e-07
gelu-dw1-2^24       32x40  f32 1.6e-06 | before 2/2/2 6.5e-06 | after 2/2/2 3.3e-07
gelu-dw2-2^-24      32x40  f32 1.6e-06 | before 2/2/2 7.7e-05 | after 2/2/2 3.3e-07
gelu-dw2-2^24       32x40  f32 1.6e-06 | before 2/2/2 4.1e-06 | after 2/2/2 3.3e-07
gelu-dw3-2^-24      32x40  f32 1.6e-06 | before 2/2/2 1.5e-05 | after 2/2/2 3.3e-07
gelu-dw3-2^24       32x40  f32 1.6e-06 | before 2/2/2 1.6e-05 | after 2/2/2 3.3e-07
silu-dw1-2^-24      32x40  f32 1.9e-06 | before 2/2/2 2.1e-05 | after 2/2/2 2.7e-07
silu-dw1-2^24       32x40  f32 1.9e-06 | before 2/2/2 1.1e-05 | after 2/2/2 2.7e-07
silu-dw2-2^-24      32x40  f32 1.9e-06 | before 2/2/2 7.7e-05 | after 2/2/2 2.7e-07
silu-dw2-2^24       32x40  f32 1.9e-06 | before 2/2/2 4.8e-06 | after 2/2/2 2.7e-07
silu-dw3-2^-24      32x40  f32 1.9e-06 | before 2/2/2 1.9e-05 | after 2/2/2 2.7e-07
silu-dw3-2^24       32x40  f32 1.9e-06 | before 2/2/2 1.6e-05 | after 2/2/2 2.7e-07
gelu-l0-2^12        32x40  f32 1.4e-06 | before 2/2/2 2.5e-07 | after 2/2/2 2.5e-07
gelu-l0-2^-12       32x40  f32 1.7e-06 | before 2/2/2 3.2e-07 | after 2/2/2 3.2e-07
gelu-l0-2^16        32x40  f32 1.4e-06 | before 2/2/2 3.2e-07 | after 3/2/2 2.9e-07
gelu-l0-2^-16       32x40  f32 1.8e-06 | before 2/2/2 3.4e-07 | after 3/2/2 3.3e-07
gelu-l0-2^20        32x40  f32 1.4e-06 | before 2/2/2 1.1e-06 | after 3/2/2 2.9e-07
gelu-l0-2^-20       32x40  f32 2.2e-06 | before 2/2/2 2.7e-06 | after 3/2/2 3.4e-07
gelu-l0-2^24        32x40  f32 1.4e-06 | before 2/2/2 1.4e-05 | after 3/2/2 2.9e-07
gelu-l0-2^-24       32x40  f32 1.8e-06 | before 2/2/2 6.1e-05 | after 3/2/2 2.8e-07
gelu-l1-2^12        32x40  f32 1.9e-06 | before 2/2/2 3.0e-07 | after 2/2/2 3.0e-07
gelu-l1-2^-12       32x40  f32 1.4e-06 | before 2/2/2 3.2e-07 | after 2/2/2 3.2e-07
gelu-l1-2^16        32x40  f32 1.9e-06 | before 2/2/2 2.9e-07 | after 2/3/2 2.3e-07
gelu-l1-2^-16       32x40  f32 3.0e-06 | before 2/2/2 2.3e-07 | after 2/3/2 2.6e-07
gelu-l1-2^20        32x40  f32 1.9e-06 | before 2/2/2 5.8e-07 | after 2/3/2 2.3e-07
gelu-l1-2^-20       32x40  f32 1.6e-06 | before 2/2/2 2.5e-06 | after 2/3/2 2.0e-07
gelu-l1-2^24        32x40  f32 1.9e-06 | before 2/2/2 4.6e-06 | after 2/3/2 2.3e-07
gelu-l1-2^-24       32x40  f32 1.9e-06 | before 2/2/2 8.4e-05 | after 2/3/2 2.6e-07
gelu-l2-2^12        32x40  f32 1.6e-06 | before 2/2/2 3.2e-07 | after 2/2/2 3.2e-07
gelu-l2-2^-12       32x40  f32 1.6e-06 | before 2/2/2 3.0e-07 | after 2/2/2 3.0e-07
gelu-l2-2^16        32x40  f32 1.6e-06 | before 2/2/2 3.6e-07 | after 2/2/3 3.6e-07
gelu-l2-2^-16       32x40  f32 1.7e-06 | before 2/2/2 2.0e-07 | after 2/2/3 3.4e-07
gelu-l2-2^20        32x40  f32 1.6e-06 | before 2/2/2 1.4e-06 | after 2/2/3 3.6e-07
gelu-l2-2^-20       32x40  f32 1.1e-06 | before 2/2/2 4.4e-06 | after 2/2/3 3.4e-07
gelu-l2-2^24        32x40  f32 1.6e-06 | before 2/2/2 2.1e-05 | after 2/2/3 3.6e-07
gelu-l2-2^-24       32x40  f32 1.3e-06 | before 2/2/2 2.3e-05 | after 2/2/3 3.4e-07
silu-l0-2^12        32x40  f32 1.5e-06 | before 2/2/2 3.1e-07 | after 2/2/2 3.1e-07
silu-l0-2^-12       32x40  f32 2.0e-06 | before 2/2/2 2.9e-07 | after 2/2/2 2.9e-07
silu-l0-2^16        32x40  f32 1.5e-06 | before 2/2/2 3.5e-07 | after 3/2/2 3.5e-07
silu-l0-2^-16       32x40  f32 1.9e-06 | before 2/2/2 2.3e-07 | after 3/2/2 3.6e-07
silu-l0-2^20        32x40  f32 1.5e-06 | before 2/2/2 6.1e-07 | after 3/2/2 3.5e-07
silu-l0-2^-20       32x40  f32 2.3e-06 | before 2/2/2 3.1e-06 | after 3/2/2 3.4e-07
silu-l0-2^24        32x40  f32 1.5e-06 | before 2/2/2 1.3e-05 | after 3/2/2 3.5e-07
silu-l0-2^-24       32x40  f32 1.7e-06 | before 2/2/2 6.5e-05 | after 3/2/2 3.1e-07
silu-l1-2^12        32x40  f32 1.3e-06 | before 2/2/2 2.4e-07 | after 2/2/2 2.4e-07
silu-l1-2^-12       32x40  f32 2.0e-06 | before 2/2/2 3.1e-07 | after 2/2/2 3.1e-07
silu-l1-2^16        32x40  f32 1.3e-06 | before 2/2/2 2.4e-07 | after 2/3/2 2.0e-07
silu-l1-2^-16       32x40  f32 1.7e-06 | before 2/2/2 2.6e-07 | after 2/3/2 1.7e-07
silu-l1-2^20        32x40  f32 1.3e-06 | before 2/2/2 4.4e-07 | after 2/3/2 2.0e-07
silu-l1-2^-20       32x40  f32 2.3e-06 | before 2/2/2 2.7e-06 | after 2/3/2 2.1e-07
silu-l1-2^24        32x40  f32 1.3e-06 | before 2/2/2 5.0e-06 | after 2/3/2 2.0e-07
silu-l1-2^-24       32x40  f32 1.8e-06 | before 2/2/2 7.9e-05 | after 2/3/2 2.0e-07
silu-l2-2^12        32x40  f32 1.8e-06 | before 2/2/2 2.6e-07 | after 2/2/2 2.6e-07
silu-l2-2^-12       32x40  f32 1.4e-06 | before 2/2/2 2.5e-07 | after 2/2/2 2.5e-07
silu-l2-2^16        32x40  f32 1.8e-06 | before 2/2/2 2.7e-07 | after 2/2/3 3.1e-07
silu-l2-2^-16       32x40  f32 1.3e-06 | before 2/2/2 2.6e-07 | after 2/2/3 2.6e-07
silu-l2-2^20        32x40  f32 1.8e-06 | before 2/2/2 1.2e-06 | after 2/2/3 3.1e-07
silu-l2-2^-20       32x40  f32 1.4e-06 | before 2/2/2 4.7e-06 | after 2/2/3 2.6e-07
silu-l2-2^24        32x40  f32 1.8e-06 | before 2/2/2 1.9e-05 | after 2/2/3 3.1e-07
silu-l2-2^-24       32x40  f32 1.3e-06 | before 2/2/2 2.0e-05 | after 2/2/3 2.6e-07

numpy only: nothing here loads the native library."""
import functools
import math

import numpy as np
import pytest

from nanowakeword_amd.config import HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from oracle import heads as oh
import oracle
from test_trunk_stress import (BAR, FEATURE_BOUND, FEATURE_TYP, MEAN_LOG2, _split, bars_ok, f16_rows, f16_rows_seen, f16_rows_typ, f16_scale,
                               f16_wscale, rel_err)

SHAPES = ((32, 40), (70, 64))           # block-3 planes of 2 x 5 = 10 pixels (one ragged group) and 5 x 8 = 40 (two, the second ragged)
BATCH = 33
GS = (8, 12, 16, 20, 24)
GS_LARGE = (20, 24)                     # the rows kept at SHAPES[1]
CH_A, CH_B = 3, 5
CHANNELS = (32, 64, 128, 256)
STRIDES = ((2, 2), (2, 2), (2, 1))
PIXEL_LOG2 = MEAN_LOG2                  # f16_pixel_rows_ok's window: f16_range_factor()


def config(shape, activation="relu"):
    return HeadConfig("bcresnet", shape, activation=activation)


# ---- the rescales
def rescale(sd, link, channel, g):
    """one link's channel x 2^g and what reads it / 2^g -> a new state dict.  "l0" .. "l3": BatchNorm weight and bias (both BatchNorms of a
    block together); "dw1" .. "dw3": the depthwise row against the pointwise column"""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    G = np.float32(2.0 ** g)
    if link.startswith("dw"):
        i = int(link[2:])
        out[f"model.block{i}.depthwise.weight"][channel] *= G
        out[f"model.block{i}.pointwise.weight"][:, channel] /= G
        return out
    i = int(link[1:])
    bns = ("model.init_conv.1",) if i == 0 else (f"model.block{i}.bn1", f"model.block{i}.shortcut.1")
    for bn in bns:
        out[bn + ".weight"][channel] *= G
        out[bn + ".bias"][channel] *= G
    if i < 3:
        out[f"model.block{i + 1}.pointwise.weight"][:, channel] /= G
        out[f"model.block{i + 1}.shortcut.0.weight"][:, channel] /= G
    else:
        out["model.fc.weight"][:, channel] /= G
    return out


LINKS = ("l0", "l1", "l2", "l3", "dw1", "dw2", "dw3")
RESCALE = {}                            # name -> ((link, channel, g), ...): ReLU, the same function
for _g in GS:
    for _s in (1, -1):
        for _l in LINKS:
            RESCALE[f"{_l}-2^{_s * _g}"] = ((_l, CH_A, _s * _g),)
        RESCALE[f"l01-2^{_s * _g}"] = (("l0", CH_A, _s * _g), ("l1", CH_B, _s * _g))
# the depthwise links under the other activations: still the same function, still balanced
DW_ANY = {f"{a}-{l}-2^{g}": (a, ((l, CH_A, g),)) for a in ("gelu", "silu") for l in ("dw1", "dw2", "dw3") for g in (-24, 24)}
# GELU / SiLU BatchNorm links: not the same function, cannot be balanced; the guard decides.  name -> (activation, steps)
UNBALANCED = {f"{a}-{l}-2^{s * g}": (a, ((l, CH_A, s * g),)) for a in ("gelu", "silu") for l in ("l0", "l1", "l2") for g in (12, 16, 20, 24) for s in (1, -1)}
DATA = {"x2^-10": -10, "x2^-5": -5, "x2^5": 5}
MIXED_CLIP, MIXED_EXP = 5, -10


def names_at(shape):
    """the RESCALE rows a shape runs: all of them at SHAPES[0], +-20 and +-24 at SHAPES[1]"""
    return [n for n, steps in RESCALE.items() if shape == SHAPES[0] or all(abs(g) in GS_LARGE for _, _, g in steps)]


def unbalanced_at(shape):
    return [n for n, (_, steps) in UNBALANCED.items() if shape == SHAPES[0] or all(abs(g) in GS_LARGE for _, _, g in steps)]


CASES = [(n, s) for s in SHAPES for n in names_at(s)]
UNBALANCED_CASES = [(n, s) for s in SHAPES for n in unbalanced_at(s)]
_case_ids = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]


@functools.lru_cache(maxsize=None)
def base_case(shape, activation="relu"):
    """-> (cfg, synth_state_dict, features [BATCH, *shape], float64 logits, float32 oracle logits): evaluated once, read-only"""
    cfg = config(shape, activation)
    sd = synth_state_dict(cfg)
    feats = synth_features(BATCH, shape, seed=9)
    l64 = oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel()
    l32 = oracle.model_forward(feats, sd, cfg).ravel()
    for a in (feats, l64, l32, *sd.values()):
        a.setflags(write=False)
    return cfg, sd, feats, l64, l32


@functools.lru_cache(maxsize=None)
def case_sd(name, shape):
    """-> (cfg, state dict) of a RESCALE, DW_ANY or UNBALANCED case, or of the plain weights (name = an activation)"""
    if name in ("relu", "gelu", "silu"):
        activation, steps = name, ()
    elif name in RESCALE:
        activation, steps = "relu", RESCALE[name]
    else:
        activation, steps = (DW_ANY if name in DW_ANY else UNBALANCED)[name]
    cfg, sd = base_case(shape, activation)[:2]
    for link, channel, g in steps:
        sd = rescale(sd, link, channel, g)
    for a in sd.values():
        a.setflags(write=False)
    return cfg, sd


def data_feats(name, shape):
    feats = synth_features(BATCH, shape, seed=9) * np.float32(2.0 ** DATA[name])
    assert np.abs(feats).max() < FEATURE_BOUND
    return feats


def mixed_feats(shape):
    feats = synth_features(BATCH, shape, seed=9)
    feats[MIXED_CLIP] *= np.float32(2.0 ** MIXED_EXP)
    return feats


def loud_frame_feats(shape):
    """one clip x 2^-10 with a single frame left at full scale (the Conformer suite's quiet-clip case)"""
    feats = synth_features(BATCH, shape, seed=9)
    keep = feats[MIXED_CLIP, shape[0] // 2].copy()
    feats[MIXED_CLIP] *= np.float32(2.0 ** MIXED_EXP)
    feats[MIXED_CLIP, shape[0] // 2] = keep
    return feats


# ---- the library's arithmetic on the weights' values (plan_host.h, nww_weights.hip, nww_plan.hip), in float64 as there
def fold(sd, bn):
    """fold_batchnorms: float32, alpha = w / sqrt(var + eps), beta = b - mean alpha"""
    inv = np.float32(1.0) / np.sqrt(np.asarray(sd[bn + ".running_var"], np.float32) + np.float32(1e-5))
    al = (np.asarray(sd[bn + ".weight"], np.float32) * inv).astype(np.float32)
    return al, (np.asarray(sd[bn + ".bias"], np.float32) - np.asarray(sd[bn + ".running_mean"], np.float32) * al).astype(np.float32)


BALANCE_MIN_LOG2, BALANCE_MAX_LOG2 = 4.0, 40.0


def _balance_channels(out, producers, in_bounds, consumers):
    """balance_channels (plan_host.h) on the state dict `out`, in place on copies: producers = [(conv key prefix, BatchNorm prefix or None)]
    whose outputs are ADDED into one channel (its bound: the sum of theirs, each on its own input bound; all take the same 2^e), consumers =
    the weight keys that read the channel in column blocks -> the largest channel bound after"""
    t = 0.0
    for (conv, bn), in_bound in zip(producers, in_bounds):
        w = np.asarray(out[conv + ".weight"], np.float64)
        b = np.abs(w.reshape(w.shape[0], -1)).sum(1) * in_bound
        if conv + ".bias" in out:
            b = b + np.abs(np.asarray(out[conv + ".bias"], np.float64))
        if bn:
            al = np.asarray(out[bn + ".weight"], np.float64) / np.sqrt(np.asarray(out[bn + ".running_var"], np.float64) + 1e-5)
            b = b * np.abs(al) + np.abs(np.asarray(out[bn + ".bias"], np.float64) - np.asarray(out[bn + ".running_mean"], np.float64) * al)
        t = t + b
    C = len(t)
    q = np.zeros(C)
    for k in consumers:
        wn = np.asarray(out[k], np.float64).reshape(out[k].shape[0], -1)
        q += (wn.reshape(wn.shape[0], C, -1) ** 2).sum(axis=(0, 2))
    worth = t * np.sqrt(q)
    counts = (worth > 0) & (worth >= worth[np.isfinite(worth)].max(initial=0.0) * 2.0 ** -8)
    med = np.sort(t[counts])[counts.sum() // 2] if counts.any() else 0.0
    exps = np.zeros(C, int)
    for c in range(C):
        if med > 0 and counts[c] and np.isfinite(t[c]):
            l = math.log2(t[c] / med)
            if BALANCE_MIN_LOG2 <= abs(l) <= BALANCE_MAX_LOG2:
                exps[c] = -int(math.copysign(math.floor(abs(l) + 0.5), l))
    if exps.any():
        keys = []
        for conv, bn in producers:
            keys += [bn + ".weight", bn + ".bias"] if bn else [conv + ".weight"] + ([conv + ".bias"] if conv + ".bias" in out else [])
        for k in keys + list(consumers):
            out[k] = np.array(out[k], np.float32, copy=True)
        for c in np.nonzero(exps)[0]:
            for k in keys:
                out[k][c] *= np.float32(2.0 ** exps[c])
            for k in consumers:
                flat = out[k].reshape(out[k].shape[0], -1)                  # a view: channel c is columns c per .. c per + per - 1
                per = flat.shape[1] // C
                flat[:, c * per:(c + 1) * per] *= np.float32(2.0 ** -exps[c])
    return float((t * 2.0 ** exps).max())


def balance(sd, cfg):
    """balance_channel_gains for this head (nww_weights.hip), on the loaded weights before the BatchNorms are folded: per i = 0 .. 3, under
    ReLU the channels of h_i - the init conv's BatchNorm, or block i's bn1 and shortcut.1 as one channel - against block i + 1's pointwise
    and shortcut.0 columns (fc.weight behind block 3); then, under every activation, block i + 1's depthwise rows against its pointwise
    columns.  -> a new state dict (the input's arrays where nothing moved)"""
    out = dict(sd)
    bound_h = FEATURE_BOUND
    for i in range(4):
        q, qn = f"model.block{i}", f"model.block{i + 1}"
        if cfg.activation == "relu":
            if i == 0:
                prod, ins = [("model.init_conv.0", "model.init_conv.1")], [bound_h]
            else:
                dw = np.abs(np.asarray(out[q + ".depthwise.weight"], np.float64)).reshape(CHANNELS[i - 1], 9)
                prod, ins = [(q + ".pointwise", q + ".bn1"), (q + ".shortcut.0", q + ".shortcut.1")], [float(dw.sum(1).max()) * bound_h, bound_h]
            cons = [qn + ".pointwise.weight", qn + ".shortcut.0.weight"] if i < 3 else ["model.fc.weight"]
            bound_h = _balance_channels(out, prod, ins, cons)
        if i < 3:
            _balance_channels(out, [(qn + ".depthwise", None)], [1.0], [qn + ".pointwise.weight"])
    return out


def pixel_rows_ok(w, typ):
    """f16_pixel_rows_ok (plan_host.h): w [Cout, K] read on an operand whose channels have the typical magnitudes typ [K].  The operand's
    absolute error is 2^-39 of its row's largest element, the weights' 2^-39 of the tensor's largest: both against each output row"""
    w = np.asarray(w, np.float64)
    typ = np.asarray(typ, np.float64)
    sig2, norm2 = f16_rows(w, typ)
    tmax, t2 = float(typ.max()), float((typ ** 2).sum())
    if not tmax > 0 or not math.isfinite(t2):
        return False
    window, seen = 2.0 ** PIXEL_LOG2, f16_rows_seen(sig2, norm2)
    if not seen < math.inf or not tmax <= seen * window:
        return False
    live = norm2 > 0
    return bool((np.abs(w).max() * math.sqrt(t2) <= np.sqrt(sig2[live]) * window).all())


def dual_x3_mean_supported(pixels):
    return 1 <= pixels <= 128 and 4 % ((pixels + 31) // 32) == 0


def out_plane(hw, stride):
    return (hw[0] - 1) // stride[0] + 1, (hw[1] - 1) // stride[1] + 1


def plan(sd, cfg, guard="rows"):
    """plan_bcresnet's decisions on the weights' values -> dict(front: the init conv on two terms, blocks: per block, its two products on
    two terms; f_in, f_w0, ws: the scales; mean_fused).  guard = "none": before this file (no guard), "rows": f16_pixel_rows_ok per block
    on the per-channel typical magnitudes (f16_rows_typ through the float32 folded BatchNorms, a block's two branches by hypot)"""
    w0 = np.asarray(sd["model.init_conv.0.weight"], np.float32).reshape(32, 9)
    al0, be0 = fold(sd, "model.init_conv.1")
    typ_h = f16_rows_typ(f16_rows(w0, [FEATURE_TYP])[0], dict(b=np.zeros(32, np.float32), al=al0, be=be0))
    blocks, ws = [], []
    hw = (cfg.input_shape[0] // 2, cfg.input_shape[1] // 2)
    for i in (1, 2, 3):
        q = f"model.block{i}"
        ci, co = CHANNELS[i - 1], CHANNELS[i]
        dw = np.asarray(sd[q + ".depthwise.weight"], np.float64).reshape(ci, 9)
        typ_d = np.sqrt((dw ** 2).sum(1)) * typ_h
        wpw, wsc = np.asarray(sd[q + ".pointwise.weight"], np.float32).reshape(co, ci), np.asarray(sd[q + ".shortcut.0.weight"], np.float32).reshape(co, ci)
        blocks.append(guard == "none" or (pixel_rows_ok(wpw, typ_d) and pixel_rows_ok(wsc, typ_h)))
        ws.append((f16_wscale(wpw), f16_wscale(wsc)))
        (a1, b1), (a2, b2) = fold(sd, q + ".bn1"), fold(sd, q + ".shortcut.1")
        zero = np.zeros(co, np.float32)
        typ_h = np.hypot(f16_rows_typ(f16_rows(wpw, typ_d)[0], dict(b=zero, al=a1, be=b1)), f16_rows_typ(f16_rows(wsc, typ_h)[0], dict(b=zero, al=a2, be=b2)))
        hw = out_plane(hw, STRIDES[i - 1])
    return dict(front=True, blocks=tuple(blocks), f_in=f16_scale(FEATURE_BOUND), f_w0=f16_wscale(w0), ws=ws, mean_fused=dual_x3_mean_supported(hw[0] * hw[1]))


def forms(p):
    return "/".join("2" if b else "3" for b in p["blocks"])


# ---- the two-term arithmetic
def _row_scale(m):
    """the power of two of a row whose largest magnitude is m (float32): eb = clamp(biased exponent, 16, 254), 2^(141 - eb)"""
    eb = np.clip(np.asarray(m, np.float32).view(np.uint32) >> 23, 16, 254).astype(np.int64)
    return np.ldexp(1.0, 141 - eb)


def _rows2(x, w, srow, ws):
    """x [M, K] under a scale per row, w [N, K] under one scale: hi hi + lo hi + hi lo (binary16 products are exact in the float32
    accumulator, whose own rounding the float64 sum here leaves out)"""
    xh, xl = _split(np.asarray(x, np.float64).astype(np.float32) * srow[:, None].astype(np.float32))
    wh, wl = _split(np.asarray(w, np.float32) * np.float32(ws))
    return (xh @ wh.T + xl @ wh.T + xh @ wl.T) / (srow[:, None] * float(ws))


def _front2(x, w, xs, ws):
    xh, xl = _split(np.asarray(x, np.float64).astype(np.float32) * np.float32(xs))
    wh, wl = _split(np.asarray(w, np.float32) * np.float32(ws))
    return (oh.conv2d(xh, wh) + oh.conv2d(xl, wh) + oh.conv2d(xh, wl)) / (float(xs) * float(ws))


def forward(feats, sd, cfg, p=None):
    """the head in float64 with the float32 BatchNorm folds the device uses; with a plan p, the operands the device splits go through the
    two-term arithmetic under the scales it takes: the front kernel's features and weights, and per block on two terms the rows of d and of
    xs (per pixel; per 32-pixel group of a clip in the last block when the mean is fused) and Wpw, Wsc.  A block on three terms is exact"""
    a = cfg.activation
    h = np.asarray(feats, np.float64)[:, None]
    w0 = np.asarray(sd["model.init_conv.0.weight"], np.float32)
    if p and p["front"]:
        y = _front2(np.clip(h, -FEATURE_BOUND, FEATURE_BOUND), w0, p["f_in"], p["f_w0"])
    else:
        y = oh.conv2d(h, w0.astype(np.float64))
    al, be = fold(sd, "model.init_conv.1")
    h = oh.maxpool2(oh.act(y * al.astype(np.float64).reshape(1, -1, 1, 1) + be.astype(np.float64).reshape(1, -1, 1, 1), a))
    for i, stride in zip((1, 2, 3), STRIDES):
        q = f"model.block{i}"
        wpw, wsc = np.asarray(sd[q + ".pointwise.weight"], np.float32)[:, :, 0, 0], np.asarray(sd[q + ".shortcut.0.weight"], np.float32)[:, :, 0, 0]
        d = oh.conv2d(h, np.asarray(sd[q + ".depthwise.weight"], np.float64), None, stride, (1, 1), groups=h.shape[1])
        xs = h[:, :, ::stride[0], ::stride[1]]
        B, C, Ho, Wo = d.shape
        rows = lambda t: np.ascontiguousarray(t.transpose(0, 2, 3, 1)).reshape(B * Ho * Wo, C)
        dr, xr = rows(d), rows(xs)
        if p and p["blocks"][i - 1]:
            ys = []
            for r, w, s in ((dr, wpw, p["ws"][i - 1][0]), (xr, wsc, p["ws"][i - 1][1])):
                m = np.abs(r.astype(np.float32)).max(1)
                if i == 3 and p["mean_fused"]:          # one scale per 32-pixel group of a clip, over its valid pixels
                    m = m.reshape(B, Ho * Wo)
                    for g0 in range(0, Ho * Wo, 32):
                        m[:, g0:g0 + 32] = m[:, g0:g0 + 32].max(1, keepdims=True)
                    m = m.reshape(-1)
                ys.append(_rows2(r, w, _row_scale(m), s))
            ypw, ysc = ys
        else:
            ypw, ysc = dr @ wpw.astype(np.float64).T, xr @ wsc.astype(np.float64).T
        (a1, b1), (a2, b2) = fold(sd, q + ".bn1"), fold(sd, q + ".shortcut.1")
        o = oh.act(ypw * a1.astype(np.float64) + b1.astype(np.float64), a) + (ysc * a2.astype(np.float64) + b2.astype(np.float64))
        h = o.reshape(B, Ho, Wo, -1).transpose(0, 3, 1, 2)
    e = oh.linear(h.mean(axis=(2, 3)), np.asarray(sd["model.fc.weight"], np.float64), np.asarray(sd["model.fc.bias"], np.float64))
    return oracle.classify(e, sd, cfg, dtype=np.float64).ravel()


@functools.lru_cache(maxsize=None)
def emulated(name, shape, mode):
    """-> (plan, the emulator's error under it, the float32 oracle's error, the float64 logits) of a case.  mode "before": the weights as
    given, no guard; "after": balanced, then guarded"""
    cfg, sd = case_sd(name, shape)
    feats = base_case(shape)[2]
    l64 = oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel()
    f32 = rel_err(oracle.model_forward(feats, sd, cfg).ravel(), l64)
    if mode == "after":
        sd = balance(sd, cfg)
    p = plan(sd, cfg, "none" if mode == "before" else "rows")
    return p, rel_err(forward(feats, sd, cfg, p), l64), f32, l64


def _row(name, shape):
    (po, eo, f32, _), (pn, en, _, _) = emulated(name, shape, "before"), emulated(name, shape, "after")
    return f"{name:18s} {shape[0]:3d}x{shape[1]:<3d} f32 {f32:.1e} | before {forms(po)} {eo:.1e} | after {forms(pn)} {en:.1e}"


def table(shapes=SHAPES):
    """the docstring's table (python -c "import test_bcresnet_stress as t; print(t.table())" from tests/)"""
    out = []
    for s in shapes:
        out += [_row(n, s) for n in ["relu", "gelu", "silu"] + names_at(s) + list(DW_ANY) + unbalanced_at(s)]
    return "\n".join(out)


# ---- the tests
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("activation", ["relu", "gelu", "silu"])
def test_forward_restates_the_oracle(activation, shape):
    """forward() without a plan is the float64 oracle to the rounding of the float32 BatchNorm folds (one rounding of alpha and of beta per
    channel and BatchNorm, 6e-8 each)"""
    cfg, sd, feats, l64, _ = base_case(shape, activation)
    d = rel_err(forward(feats, sd, cfg), l64)
    print(f"bcresnet {activation} {shape}: forward() without a plan vs the float64 oracle {d:.2e}")
    assert d <= 5e-7, (activation, shape, d)


@pytest.mark.parametrize("name,shape", CASES, ids=_case_ids)
def test_rescale_preserves_the_function(name, shape):
    """float32 oracle: the same bits as on the plain weights; float64: 1e-12 relative.  And the case is no vacuous one: logit ptp > 1e-2
    and the float32 oracle within a tenth of the 1e-4 bar of float64"""
    cfg, _, feats, l64, l32 = base_case(shape)
    sd = case_sd(name, shape)[1]
    assert np.array_equal(oracle.model_forward(feats, sd, cfg).ravel(), l32), name
    assert np.abs(oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel() - l64).max() <= 1e-12 * max(1.0, np.abs(l64).max()), name
    assert np.ptp(l64) > 1e-2 and rel_err(l32, l64) <= BAR / 10, (name, float(np.ptp(l64)), rel_err(l32, l64))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(DW_ANY))
def test_depthwise_rescale_preserves_the_function_under_any_activation(name, shape):
    """nothing nonlinear sits between a block's depthwise and its pointwise: the same float32 bits under GELU and SiLU too"""
    activation = DW_ANY[name][0]
    cfg, _, feats, l64, l32 = base_case(shape, activation)
    sd = case_sd(name, shape)[1]
    assert np.array_equal(oracle.model_forward(feats, sd, cfg).ravel(), l32), name
    assert np.abs(oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel() - l64).max() <= 1e-12 * max(1.0, np.abs(l64).max()), name
    assert np.ptp(l64) > 1e-2 and rel_err(l32, l64) <= BAR / 10, (name, float(np.ptp(l64)), rel_err(l32, l64))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("activation", ["relu", "gelu", "silu"])
def test_plain_weights_and_data_cases(activation, shape):
    """plain weights: the guard keeps every block on two terms and the balance moves nothing, and the emulator is inside the bars on the
    plain clips, on whole batches x 2^-10 / 2^-5 / 2^5, on one quiet clip among ordinary ones and on a quiet clip with one frame at full
    scale (every scale is taken inside a clip: the quiet clip's logit is the one it has alone)"""
    cfg, sd, feats, l64, l32 = base_case(shape, activation)
    bal = balance(sd, cfg)
    assert all(bal[k] is sd[k] for k in sd), activation
    p = plan(sd, cfg)
    assert p["blocks"] == (True, True, True) and p["mean_fused"], p
    cases = [("plain", feats)] + [(n, data_feats(n, shape)) for n in DATA] + [("mixed", mixed_feats(shape)), ("loud frame", loud_frame_feats(shape))]
    for what, x in cases:
        ref = oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
        f32 = rel_err(oracle.model_forward(x, sd, cfg).ravel(), ref)
        got = forward(x, sd, cfg, p)
        err = rel_err(got, ref)
        print(f"bcresnet {activation} {shape} {what}: emulated {err:.2e}, float32 oracle {f32:.2e}, |logit|max {np.abs(ref).max():.3g}, ptp {np.ptp(ref):.3g}")
        # no vacuous case: the plain clips spread their logits over > 1e-2 like every rescaled case, the quiet batches (|logit| < 1, so the
        # error is absolute there) over a hundred times the bar they are held to
        assert np.ptp(ref) > (1e-2 if what == "plain" else 1e2 * (2.0 * f32 + 2e-6)), (activation, shape, what, float(np.ptp(ref)))
        assert f32 <= BAR / 10 and bars_ok(err, f32), (activation, shape, what, err, f32)
        if what in ("mixed", "loud frame"):
            alone = forward(x[MIXED_CLIP:MIXED_CLIP + 1], sd, cfg, p)
            assert abs(alone[0] - got[MIXED_CLIP]) <= 1e-12 * max(1.0, abs(alone[0]))


@pytest.mark.parametrize("name,shape", CASES, ids=_case_ids)
def test_balanced_models_keep_the_two_term_kernels(name, shape):
    """what the library makes of a ReLU model before it plans (balance): still the same function with the same float32 bits, planned on
    two terms throughout (2^8 and 2^24 alike), and the emulator on it inside the bars"""
    cfg, _, feats, l64, l32 = base_case(shape)
    bal = balance(case_sd(name, shape)[1], cfg)
    assert np.array_equal(oracle.model_forward(feats, bal, cfg).ravel(), l32), name
    p, err, f32, _ = emulated(name, shape, "after")
    print(f"{name} {shape} balanced and guarded: blocks {forms(p)}, emulated {err:.2e}, float32 {f32:.2e}")
    assert p["blocks"] == (True, True, True), (name, p)
    assert bars_ok(err, f32), (name, err, f32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(DW_ANY))
def test_depthwise_links_are_balanced_under_any_activation(name, shape):
    activation = DW_ANY[name][0]
    cfg, _, feats, l64, l32 = base_case(shape, activation)
    bal = balance(case_sd(name, shape)[1], cfg)
    assert np.array_equal(oracle.model_forward(feats, bal, cfg).ravel(), l32), name
    p, err, f32, _ = emulated(name, shape, "after")
    print(f"{name} {shape} balanced and guarded: blocks {forms(p)}, emulated {err:.2e}, float32 {f32:.2e}")
    assert p["blocks"] == (True, True, True), (name, p)
    assert bars_ok(err, f32), (name, err, f32)


@pytest.mark.parametrize("name,shape", UNBALANCED_CASES, ids=[f"{n}-{s[0]}x{s[1]}" for n, s in UNBALANCED_CASES])
def test_guard_leaves_only_sound_cases(name, shape):
    """GELU / SiLU BatchNorm links cannot be balanced (nothing of them moves: only a depthwise row may); every block the guard leaves on
    the two-term form is emulated inside the bars, judged against float64 on the case's own weights, and the case is no vacuous one"""
    cfg, sd = case_sd(name, shape)
    bal = balance(sd, cfg)
    assert all(bal[k] is sd[k] for k in sd if "depthwise" not in k and "pointwise" not in k), name
    p, err, f32, l64 = emulated(name, shape, "after")
    print(f"{name} {shape} guarded: blocks {forms(p)}, emulated {err:.2e}, float32 {f32:.2e}")
    assert np.ptp(l64) > 1e-2 and f32 <= BAR / 10, (name, float(np.ptp(l64)), f32)
    assert bars_ok(err, f32), (name, shape, err, f32)


# where the unguarded, unbalanced plan leaves the bars at SHAPES[0] (the table's "before" column)
TEETH = ["l0-2^24", "l0-2^-24", "l1-2^-24", "l2-2^24", "l2-2^-24", "dw2-2^-24", "dw3-2^24", "l01-2^-24",
         "gelu-dw2-2^-24", "gelu-l0-2^-24", "gelu-l1-2^-24", "silu-l2-2^24"]


@pytest.mark.parametrize("name", TEETH)
def test_cases_have_teeth(name):
    """before this file the planner kept these on two terms throughout and the emulator is outside the bars there; now the ReLU ones are
    balanced back onto the plain weights' arithmetic and the others have the offending block on three terms - inside the bars either way"""
    po, eo, f32, _ = emulated(name, SHAPES[0], "before")
    pn, en, _, _ = emulated(name, SHAPES[0], "after")
    print(_row(name, SHAPES[0]))
    assert po["blocks"] == (True, True, True) and not bars_ok(eo, f32), (name, eo, f32)
    assert bars_ok(en, f32), (name, en, f32)
    if name in UNBALANCED:
        assert pn["blocks"] != (True, True, True), (name, pn)
    else:
        assert pn["blocks"] == (True, True, True), (name, pn)


def test_the_docstring_table_is_current():
    """every row of table() at SHAPES[0] stands in this file's docstring: the forms as printed, the three errors to 10 % and a digit's
    rounding (the sums go through the BLAS at hand, whose order may move a last printed digit)"""
    def parse(row):
        f = row.split()
        return f[0], (f[6], f[10]), np.array([float(f[3]), float(f[7]), float(f[11])])
    stated = {parse(r)[0]: parse(r) for r in __doc__.splitlines() if " f32 " in r and " | before " in r}
    for row in table(SHAPES[:1]).splitlines():
        name, fm, err = parse(row)
        assert name in stated, row
        assert stated[name][1] == fm and (np.abs(stated[name][2] - err) <= 0.1 * err + 6e-9).all(), (row, stated[name])
