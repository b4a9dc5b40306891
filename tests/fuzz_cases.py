"""Seeded random case lists for the shape sweeps of csrc/norm.hip, csrc/spatial.hip and the inference glue
(tests/test_gpu_norm_fuzz.py, tests/test_gpu_spatial_fuzz.py, tests/test_gpu_infer_glue.py) and of csrc/attn.hip
(tests/test_gpu_mha_fuzz.py; its float64 reference and bounds are tests/mha_reference.py), the written-out case list of the sweep of
csrc/msda.hip by plan, build and layout (tests/test_gpu_msda_fuzz.py; tests/msda_reference.py), the written-out case list of the sweep of
csrc/gconv.hip by group shape, launch plan and view (tests/test_gpu_gconv_fuzz.py), the written-out case list of the sweep of the dense
convolution's fused epilogues through every tile and backward path of csrc/conv.hip and csrc/igemm8p.hpp (tests/test_gpu_conv_epilogue_fuzz.py),
the written-out case lists of the sweeps of the loss kernels (csrc/loss.hip, csrc/loss_pixel.hpp, csrc/loss_ext/loss_ext.hip;
tests/test_gpu_loss_fuzz.py) and of the optimizer half of csrc/optim.hip with emrt_segmentation_areas (tests/test_gpu_step_fuzz.py; inputs,
float64 references and bounds of both: tests/loss_step_reference.py), the written-out case lists of the kernels that draw a dropout mask
(emrt_dropout_fwd / emrt_mask_bwd: tests/test_gpu_dropout_fuzz.py; the LayerNorm kernels with a fused branch dropout:
tests/test_gpu_norm_fuzz.py; emrt_conv2d_drop: tests/test_gpu_conv_epilogue_fuzz.py -- every mask held to tests/dropout_reference.py, the host
model of csrc/drop_hash.hpp) and of the small streaming kernels of csrc/elementwise.hip (tests/test_gpu_elementwise_fuzz.py),
and the dispatchers' shape predicates restated in Python.  No GPU and no library import: tests/test_fuzz_cases_cpu.py checks on any machine that every case lies inside its
entry point's accepted domain (no case is an expected refusal) and that every regime below keeps at least two cases, so a later edit of a
seed or a range cannot silently empty one.

A case is a tuple whose first element is its id; the generators draw with random.Random(<fixed seed>) and steer every draw towards one
regime in turn (the `kinds` lists), then the REGIMES predicates -- written against the mirrored dispatcher predicates, not against the
steering -- say what each case actually hits.  Every case stays below MAX_ELEMS elements per tensor: the cost of a case is its float64
CPU reference, not the GPU.

Regime -> case ids (regime_table() renders this text; the CPU test compares):

  batchnorm         256 threads, rows_per_pass > 1, M < rows_per_pass  bn1101-{0,6,11,12,17}
  batchnorm         256 threads, rows_per_pass > 1, M ragged against it bn1101-{1,7,13}
  batchnorm         threads = C/4, whole waves                         bn1101-{2,8,14}
  batchnorm         threads = C/4, a partial last wave                 bn1101-{3,5,9,15}
  batchnorm         C = 1024 (256 threads, one row per pass)           bn1101-{4,10,16}
  groupnorm         fused (one block per image and group)              gn1202-{0,3,4,5,6,9,10,11,12,15}
  groupnorm         two-pass because HW > 4096                         gn1202-{1,7,13}
  groupnorm         two-pass because C/G > 256                         gn1202-{2,8,14}
  groupnorm         HW = 1                                             gn1202-{3,9,15}
  groupnorm_levels  L = 1                                              gnl1303-{0,4}
  groupnorm_levels  L = 4                                              gnl1303-{1,2,5}
  groupnorm_levels  a level of one row                                 gnl1303-{2,6,7}
  groupnorm_levels  row-major kernels (C = 8 G)                        gnl1303-{0,1,4,5}
  groupnorm_levels  block per (level, image, group)                    gnl1303-{2,3,6,7}
  layernorm         C < 256 (a partial pass)                           ln1404-{0,7,9,17}
  layernorm         C = 256 (one whole pass)                           ln1404-{1,4,10,15}
  layernorm         C > 256 with a ragged last pass                    ln1404-{2,5,8,11}
  layernorm         C = 1024                                           ln1404-{3,6,12,16}
  layernorm         rows % 4 != 0                                      ln1404-{1,3,4,5,6,7,8,10,11,12,13,14,16,17}
  layernorm         rows = 1                                           ln1404-{5,8,14}
  layernorm         backward blocks loop under the block cap           ln1404-{6,15}
  layernorm         form ln(a)                                         ln1404-{0,3,6,9,12,15}
  layernorm         form ln(a+b)                                       ln1404-{1,4,7,10,13,16}
  layernorm         form ln(a+b,post)                                  ln1404-{2,5,8,11,14,17}
  resize            up on both axes                                    rs1505-{0,4,7,8,11,13,17,20}
  resize            down on both axes                                  rs1505-{1,5,14,18,19,21,23}
  resize            mixed: up on one axis, down on the other           rs1505-{2,6,9,10,12,15,22,24,25}
  resize            identity                                           rs1505-{3,16}
  resize            down with align_corners=False                      rs1505-{1,5,6,9,19,21,22,23}
  resize            1-pixel input                                      rs1505-{4,17}
  resize            1-pixel output                                     rs1505-{5,18}
  resize            NHWC, 8 channels per access (bf16)                 rs1505-{0,8,17,20,21,24}
  resize            NHWC, 4 channels per access                        rs1505-{5,7,9,13,22}
  resize            NHWC, scalar                                       rs1505-{1,2,3,4,10,14,15,16,18,23}
  resize            backward: block per source pixel                   rs1505-{0,7,13,17,20}
  resize            fp32 NCHW output and its two-kernel backward       rs1505-{6,11,12,19,25}
  resize            fused addend                                       rs1505-{2,3,5,8,13,15,16,17,21,22,23}
  maxpool           stride < k (windows overlap)                       mp1606-{0,6,11,12,17}
  maxpool           stride = k                                         mp1606-{1,4,7,9,13}
  maxpool           stride > k (pixels in no window)                   mp1606-{2,3,5,8,10,14,15,16}
  maxpool           k = 1                                              mp1606-{2,3,4,9,13,15,16}
  maxpool           k = 7                                              mp1606-{17}
  maxpool           forward 8 channels per thread, backward 4          mp1606-{3,4,8,9,13,14}
  maxpool           forward scalar, backward 4 channels per thread     mp1606-{1,2,6,7,11,12,16,17}
  maxpool           scalar both ways                                   mp1606-{0,5,10,15}
  adaptive_pool     H or W < k                                         ap1707-{0,5,10}
  adaptive_pool     non-square map                                     ap1707-{0,1,2,3,4,5,6,7,8,9,10,11,12,13}
  adaptive_pool     forward: several blocks per bin                    ap1707-{2,7,9,12}
  adaptive_pool     forward: one block per bin                         ap1707-{0,1,3,4,5,6,8,10,11,13}
  adaptive_pool     scalar path (C % 4 != 0)                           ap1707-{3,5,8,13}
  adaptive_pool     backward: two-bin table                            ap1707-{1,2,4,6,7,9,11,12}
  adaptive_pool     backward: general gather                           ap1707-{0,10}
  adaptive_pool     input is a slice of a wider buffer                 ap1707-{0,1,2,3,4,6,7,9,10,11,12}
  pyramid           one launch per direction, fp32 and bf16            py1808-{0,4,6,8}
  pyramid           one launch in fp32, per scale in bf16 (8-byte slices) py1808-{2,10}
  pyramid           per-scale fallback by the knob                     py1808-{1,3,5,7,9,11}
  mha               L = 1 (VALU kernels in every dtype)                mha1909-{0,27}
  mha               odd tile count (last k-step half padding)          mha1909-{1,2,3,4,5,6,10,11,12,16,19,20,21,22,23,28,29,30,31,32,33,37,38,39,43,46,47,48,49,50,56,57,60,61,62,63}
  mha               L % 16 = 0                                         mha1909-{6,9,12,15,18,23,26,33,36,39,42,45,50,53,68,69}
  mha               L % 16 = 1                                         mha1909-{7,10,13,16,19,24,34,37,40,43,46,51,54,55,56,57,58,59,64,65}
  mha               L % 16 = 15                                        mha1909-{5,8,11,14,17,22,25,32,35,38,41,44,49,52,62,63,66,67}
  mha               L % 4 != 0 (ragged lane quads)                     mha1909-{0,1,2,4,5,7,8,10,11,13,14,16,17,19,20,21,22,24,25,27,28,29,31,32,34,35,37,38,40,41,43,44,46,47,48,49,51,52,54,55,56,57,58,59,60,61,62,63,64,65,66,67}
  mha               ragged last forward chunk                          mha1909-{10,11,12,13,14,16,17,19,20,21,22,23,24,25,37,38,39,40,41,43,44,46,47,48,49,50,51,52,56,57,58,59,60,61,62,63,64,65,66,67}
  mha               VALU backward stages Pd in LDS                     mha1909-{0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,27,28,29,30,31,32,33,34,35,36,37,38,39,40,41,42,43,44,45,46,47,48,54,55,56,57,58,59,60,61}
  mha               VALU backward re-derives Pd                        mha1909-{22,23,24,25,26,49,50,51,52,53,62,63,64,65,66,67,68,69}
  mha               M = 1                                              mha1909-{4,14,18,28,30,32,55,66,68,69}
  mha               M not in (1, 8)                                    mha1909-{0,1,2,3,5,6,8,9,11,12,13,15,16,20,21,22,23,24,26,27,29,31,33,34,35,37,38,40,41,43,44,45,46,47,50,51,52,53,54,56,60,61,62,63,64,65}
  mha               B = 1                                              mha1909-{4,6,8,18,19,25,32,39,44,45,47,48,50,62,67}
  mha               inputs: ordinary                                   mha1909-{0,4,8,12,16,20,24,28,32,36,40,44,48,52}
  mha               inputs: peaked                                     mha1909-{1,5,9,13,17,21,25,29,33,37,41,45,49,53}
  mha               inputs: negative                                   mha1909-{2,6,10,14,18,22,26,30,34,38,42,46,50}
  mha               inputs: lastkey                                    mha1909-{3,7,11,15,19,23,27,31,35,39,43,47,51}
  mha               dropout, Pd staged in LDS                          mha1909-{54,55,56,57,58,59,60,61}
  mha               dropout, Pd re-derived                             mha1909-{62,63,64,65,66,67,68,69}
  mha               dropout, odd tile count                            mha1909-{56,57,60,61,62,63}
  mha               layout: fused                                      mha1909-{0,3,6,9,12,15,18,21,24,29,32,35,38,41,44,47,50,53,54,59,60,65,66}
  mha               layout: split                                      mha1909-{1,4,7,10,13,16,19,22,25,27,30,33,36,39,42,45,48,51,55,56,61,62,67,68}
  mha               layout: offset8                                    mha1909-{2,5,8,11,14,17,20,23,26,28,31,34,37,40,43,46,49,52,57,58,63,64,69}
  mha               dropout, layout: fused                             mha1909-{54,59,60,65,66}
  mha               dropout, layout: split                             mha1909-{55,56,61,62,67,68}
  mha               dropout, layout: offset8                           mha1909-{57,58,63,64,69}
  msda              FWD_GLOBAL, build (3, 6)                           msda2010-{37,38,39,40,41,42}
  msda              FWD_GLOBAL, build (4, 4)                           msda2010-{43,44,50,53}
  msda              FWD_GLOBAL, build (3, 4)                           msda2010-{45,46,51,52}
  msda              FWD_GLOBAL, build (1, 4)                           msda2010-{47,48,49}
  msda              FWD_LDS, build (3, 6)                              msda2010-{17,18,19,20,21,22,23,24,25,34,54,55,56,57,64,65}
  msda              FWD_LDS, build (4, 4)                              msda2010-{26,27,28,36,58,59,66,67}
  msda              FWD_LDS, build (3, 4)                              msda2010-{29,30,60,61,68,69}
  msda              FWD_LDS, build (1, 4)                              msda2010-{31,32,33,35,62,63,70,71}
  msda              FWD_BAND, build (3, 6)                             msda2010-{0,1,2,3,4,5,6,7,14}
  msda              FWD_BAND, build (4, 4)                             msda2010-{8,9,10,15}
  msda              FWD_BAND, build (3, 4)                             msda2010-{11,12,13,16}
  msda              GRAD_GLOBAL, build (3, 6)                          msda2010-{7,20,37,38,39,40,41,42}
  msda              GRAD_GLOBAL, build (4, 4)                          msda2010-{28,43,44,50}
  msda              GRAD_GLOBAL, build (3, 4)                          msda2010-{45,46,51}
  msda              GRAD_GLOBAL, build (1, 4)                          msda2010-{47,48,49}
  msda              GRAD_LDS, build (3, 6)                             msda2010-{17,18,19,21,22,23,24,25,54,55,56,57,64,65}
  msda              GRAD_LDS, build (4, 4)                             msda2010-{26,27,58,59,66,67}
  msda              GRAD_LDS, build (3, 4)                             msda2010-{29,30,60,61,68,69}
  msda              GRAD_LDS, build (1, 4)                             msda2010-{31,32,33,62,63,70,71}
  msda              GRAD_BAND, build (3, 6)                            msda2010-{0,1,2,3,4,5,6}
  msda              GRAD_BAND, build (4, 4)                            msda2010-{8,9,10}
  msda              GRAD_BAND, build (3, 4)                            msda2010-{11,12,13}
  msda              ABSMAX, build (3, 6)                               msda2010-{7,38,39,40}
  msda              ABSMAX, build (4, 4)                               msda2010-{44,50}
  msda              ABSMAX, build (3, 4)                               msda2010-{45,51}
  msda              ABSMAX, build (1, 4)                               msda2010-{47,49}
  msda              SCATTER_MF, build (3, 6)                           msda2010-{17,18,19,20,21,22,23,24,25,40,41,42,64,65}
  msda              SCATTER_MF, build (4, 4)                           msda2010-{26,27,28,44,66,67}
  msda              SCATTER_MF, build (3, 4)                           msda2010-{29,30,46,51,68,69}
  msda              SCATTER_MF, build (1, 4)                           msda2010-{31,32,33,48,70,71}
  msda              SCATTER_LDS, build (3, 6)                          msda2010-{0,1,2,3,4,5,6,7,37,38,39,54,55,56,57}
  msda              SCATTER_LDS, build (4, 4)                          msda2010-{8,9,10,43,50,58,59}
  msda              SCATTER_LDS, build (3, 4)                          msda2010-{11,12,13,45,60,61}
  msda              SCATTER_LDS, build (1, 4)                          msda2010-{47,49,62,63}
  msda              FINALIZE, build (3, 6)                             msda2010-{0,1,2,3,4,5,6,7,54,55}
  msda              FINALIZE, build (4, 4)                             msda2010-{8,9,10,58,59}
  msda              FINALIZE, build (3, 4)                             msda2010-{11,12,13,60,61}
  msda              band plan: NB = 4                                  msda2010-{0,1,2,6,7,11,14}
  msda              band plan: NB = 2                                  msda2010-{3,4,5,8,9,10,12,13,15,16}
  msda              band plan: msda_band_halo = 3 (misses)             msda2010-{1,2,9,13,15}
  msda              Lq = 1                                             msda2010-{17,26,31}
  msda              Lq % 16 = 1, Lq > 1                                msda2010-{18,21,23,25,29,30,33,38,40,43,44,45,47,50,51,62,63,67,69,71}
  msda              Lq >= 1024 behind GRAD_GLOBAL (ABSMAX)             msda2010-{7,38,39,40,44,45,47,49,50,51}
  msda              Lq >= 1024, no max |dout| scan (M = 3, 16)         msda2010-{41,42}
  msda              fp32, Lq >= 1024                                   msda2010-{38,39,45,47,49,50}
  msda              fp32, a level cut into several scatter ranges      msda2010-{39,49}
  msda              scatter ranges: msda_scatter_qsplit = 2            msda2010-{55,59,61,63}
  msda              scatter ranges: msda_scatter_qsplit = -1 or msda_scatter_cuts = 3 msda2010-{56,57}
  msda              matrix-product scatter: msda_mf_bands = 16         msda2010-{65,67,69,71}
  msda              M = 1                                              msda2010-{23,45}
  msda              M = 2                                              msda2010-{24,29,43,51,68}
  msda              M = 3                                              msda2010-{18,33,42}
  msda              M = 4                                              msda2010-{6,25,35,40,48,50,53,67}
  msda              M = 8                                              msda2010-{0,1,2,3,4,5,7,8,9,10,11,12,13,14,15,16,17,19,20,21,26,27,28,30,31,32,34,36,37,38,39,44,46,47,49,52,54,55,56,57,58,59,60,61,62,63,64,65,66,69,70,71}
  msda              M = 16                                             msda2010-{22,41}
  msda              B = 1                                              msda2010-{0,1,2,3,4,5,7,8,9,10,11,12,13,14,15,16,17,24,25,26,28,31,35,38,39,41,44,46,47,49,50,52,54,55,56,57,58,59,60,61,62,63,66,68,71}
  msda              B = 2                                              msda2010-{6,19,20,21,22,27,32,33,34,36,37,40,42,43,45,51,53,64,65,69,70}
  msda              B = 3                                              msda2010-{18,23,29,30,48,67}
  msda              dtype: f32                                         msda2010-{37,38,39,43,45,47,49,50}
  msda              dtype: bf16                                        msda2010-{0,1,2,3,4,5,6,7,8,9,10,11,12,13,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31,32,33,40,41,42,44,46,48,51,54,55,56,57,58,59,60,61,62,63,64,65,66,67,68,69,70,71}
  msda              dtype: f16                                         msda2010-{14,15,16,34,35,36,52,53}
  msda              inputs: ordinary                                   msda2010-{0,6,7,8,14,17,20,22,29,34,37,41,49,53,54,57,60,64,69}
  msda              inputs: far                                        msda2010-{1,11,23,26,30,39,42,48,50,52,56,61,68}
  msda              inputs: border                                     msda2010-{5,15,24,28,31,35,43,46,58,66,70}
  msda              inputs: bandedge                                   msda2010-{2,4,9,12,16}
  msda              inputs: centres                                    msda2010-{19,27,32,36,47}
  msda              inputs: spike                                      msda2010-{10,25,40,44,45,55,59,62,65,71}
  msda              inputs: lastquery                                  msda2010-{3,13,18,21,33,38,51,63,67}
  msda              strided, FWD_GLOBAL                                msda2010-{38,42,43,48,49,50,53}
  msda              strided, FWD_LDS                                   msda2010-{18,21,23,26,27,29,33,34,55,57,59,61,63,65,67,69,70}
  msda              strided, FWD_BAND                                  msda2010-{2,5,6,9,12,14}
  msda              strided, GRAD_GLOBAL                               msda2010-{38,42,43,48,49,50}
  msda              strided, GRAD_LDS                                  msda2010-{18,21,23,26,27,29,33,55,57,59,61,63,65,67,69,70}
  msda              strided, GRAD_BAND                                 msda2010-{2,5,6,9,12}
  msda              strided, SCATTER_MF                                msda2010-{18,21,23,26,27,29,33,42,48,65,67,69,70}
  msda              strided, SCATTER_LDS                               msda2010-{2,5,6,9,12,38,43,49,50,55,57,59,61,63}
  msda              strided, band miss path                            msda2010-{2,9,12}
  msda              refmode shared-1, GRAD_GLOBAL                      msda2010-{20,38,39,42,45,47,49}
  msda              refmode batch-1, GRAD_GLOBAL                       msda2010-{28,40,43,48,51}
  msda              refmode shared-L, GRAD_GLOBAL                      msda2010-{41,46}
  msda              refmode batch-L, GRAD_GLOBAL                       msda2010-{7,37,44,50}
  msda              refmode shared-1, GRAD_LDS                         msda2010-{17,22,25,26,31,33,54,55,58,59,60,61,62,63,64,66,68,70,71}
  msda              refmode batch-1, GRAD_LDS                          msda2010-{18,24,32,57,65}
  msda              refmode shared-L, GRAD_LDS                         msda2010-{21,23,27,56,67}
  msda              refmode batch-L, GRAD_LDS                          msda2010-{19,29,30,69}
  msda              refmode shared-1, GRAD_BAND                        msda2010-{0,2,4,10,11}
  msda              refmode batch-1, GRAD_BAND                         msda2010-{3,6,12}
  msda              refmode shared-L, GRAD_BAND                        msda2010-{1,9,13}
  msda              refmode batch-L, GRAD_BAND                         msda2010-{5,8}
  msda              dref, GRAD_GLOBAL                                  msda2010-{7,37,38,44,46,47}
  msda              dref, GRAD_LDS (msda_bwd_dref_lds = 1)             msda2010-{19,21,27,30,32}
  msda              dref, msda_bwd_dref_lds = 0 (GRAD_GLOBAL)          msda2010-{20,28}
  msda              dref on a band pyramid (GRAD_GLOBAL)               msda2010-{7}
  gconv             Cg = 4, f32                                        gconv2111-{0,3,22,26,30,40}
  gconv             Cg = 4, bf16                                       gconv2111-{1,2,16,18,21,23,38}
  gconv             Cg = 8, f32                                        gconv2111-{4,7,17,19}
  gconv             Cg = 8, bf16                                       gconv2111-{5,6,28,29}
  gconv             Cg = 16, f32                                       gconv2111-{8,11,24}
  gconv             Cg = 16, bf16                                      gconv2111-{9,10,20,27}
  gconv             Cg = 32, f32                                       gconv2111-{12,15,31}
  gconv             Cg = 32, bf16                                      gconv2111-{13,14,25,39}
  gconv             Og == Cg                                           gconv2111-{0,2,5,8,12,13,21,23,24,27,29,30,32,35,36}
  gconv             Og < Cg                                            gconv2111-{4,7,9,11,14,15,19,20,25,31,34,39}
  gconv             Og > Cg                                            gconv2111-{1,3,6,10,16,17,18,22,26,28,33,37,38,40}
  gconv             Og = 4                                             gconv2111-{0,2,4,7,9,19,20,21,23,25,30,32,39}
  gconv             Og not a power of two (12, 20)                     gconv2111-{1,3,6,10,15,16,28,31,33}
  gconv             forward: QB < 64 dividing 256                      gconv2111-{4,5,8,9,12,19,21,22,23,24,25,26,27,29,32,34,36,39}
  gconv             forward: QB not dividing 256 (idle threads)        gconv2111-{0,1,2,3,6,7,10,11,14,15,20,28,30,31,33,35,37}
  gconv             forward: exactly one full slice                    gconv2111-{13,18,38}
  gconv             forward: several slices, ragged last               gconv2111-{16,17}
  gconv             dgrad: QB < 64 dividing 256                        gconv2111-{4,5,8,9,12,16,18,22,23,25,26,27,29,38,40}
  gconv             dgrad: QB not dividing 256 (idle threads)          gconv2111-{0,1,2,7,11,15,17,28,30}
  gconv             dgrad: exactly one full slice                      gconv2111-{13,19,39}
  gconv             dgrad: several slices, ragged last                 gconv2111-{14,20}
  gconv             forward: M below one tile                          gconv2111-{0,2,3,4,6,7,8,9,10,11,12,14,15,19,20,21,24,25,26,27,28,29,30,31,33,34,35,36,37}
  gconv             forward: M % (4 PS) != 0                           gconv2111-{0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,19,20,21,22,23,24,25,26,27,28,29,30,31,32,33,34,35,36,37,38,39,40}
  gconv             forward: M % 4 != 0                                gconv2111-{0,1,2,3,4,6,9,11,15,16,19,21,22,23,24,27,28,31,35,37,38,39,40}
  gconv             forward: OW % 4 != 0 (pixels cross a row end)      gconv2111-{0,1,2,3,4,6,8,9,10,11,12,13,14,15,16,19,20,21,22,23,24,25,26,27,28,29,30,31,32,33,34,35,36,37,38,39,40}
  gconv             forward: N > 1, OH OW % 4 != 0 (pixels cross an image end) gconv2111-{0,1,3,4,6,10,13,21,22,24,26,28,29,31,32}
  gconv             dgrad: W % 4 != 0 (pixels cross a row end)         gconv2111-{0,1,2,4,8,9,11,12,13,14,15,16,19,20,22,23,25,26,27,28,29,30,38,39,40}
  gconv             dgrad: N > 1, H W % 4 != 0 (pixels cross an image end) gconv2111-{0,1,4,13,22,26,28,29}
  gconv             grid-stride: forward, no statistics                gconv2111-{38}
  gconv             grid-stride: forward with statistics               gconv2111-{40}
  gconv             grid-stride: dgrad                                 gconv2111-{39}
  gconv             stride 1                                           gconv2111-{0,1,4,5,6,8,9,11,12,13,15,16,17,18,19,20,21,22,23,26,28,29,31,32,34,35,37,38,39,40}
  gconv             stride 2                                           gconv2111-{2,3,7,10,14,24,25,27,30,33,36}
  gconv             H or W = 1                                         gconv2111-{11,15}
  gconv             H or W = 2                                         gconv2111-{13,14,20}
  gconv             stride 2 on an even size                           gconv2111-{3,7,14,24,25,30,36}
  gconv             stride 2 on an odd size                            gconv2111-{2,10,14,24,27,30,33,36}
  gconv             non-square                                         gconv2111-{0,1,2,3,4,6,8,9,10,11,13,14,15,17,19,22,23,24,25,26,27,28,29,30,32,33,35,36,37}
  gconv             input view: ld                                     gconv2111-{0,2,7,10,17,20,24,26,30,32,36}
  gconv             input view: bs                                     gconv2111-{6,8,14,22,27,33}
  gconv             input view: ld+bs                                  gconv2111-{1,3,12,25,29,35}
  gconv             output view: ld                                    gconv2111-{1,4,10,12,16,19,24,26,32,36}
  gconv             output view: bs                                    gconv2111-{2,7,14,17,21,27,33,37}
  gconv             output view: ld+bs                                 gconv2111-{6,9,15,22,28,34}
  gconv             dy view: ld                                        gconv2111-{2,8,11,14,19,21,22,26,29}
  gconv             dy view: bs                                        gconv2111-{3,9,15,20,24,27,31}
  gconv             dy view: ld+bs                                     gconv2111-{6,12,17,23,28}
  gconv             dx view: ld                                        gconv2111-{8,14,16,22,26}
  gconv             dx view: bs                                        gconv2111-{1,7,11,17,19,23,27,29}
  gconv             dx view: ld+bs                                     gconv2111-{4,9,12,20,25,28}
  gconv             all dense                                          gconv2111-{5,13,18,38,39,40}
  gconv             epilogue: none                                     gconv2111-{0,2,9,12,14,19,26,28,29,30,31,32,35,38}
  gconv             epilogue: bias                                     gconv2111-{1,8,13,17,27,33,36,39}
  gconv             epilogue: fold                                     gconv2111-{3,10,22}
  gconv             epilogue: fold+relu                                gconv2111-{7,18,25,34,37}
  gconv             epilogue: stats                                    gconv2111-{4,5,16,20,40}
  gconv             epilogue: stats+relu                               gconv2111-{11,21,24}
  gconv             epilogue: stats+bias                               gconv2111-{6,15,23}
  gconv             f16 epilogue: none                                 gconv2111-{32,35}
  gconv             f16 epilogue: bias                                 gconv2111-{33,36}
  gconv             f16 epilogue: fold+relu                            gconv2111-{34,37}
  gconv             f16 at Cg = 4                                      gconv2111-{32,37}
  gconv             f16 at Cg = 8                                      gconv2111-{33,35}
  gconv             f16 at Cg = 32                                     gconv2111-{34,36}
  gconv             backward arm: all                                  gconv2111-{0,1,4,8,11,13,14,15,16,17,20,22,23,26,27,29,30,38,39,40}
  gconv             backward arm: dx                                   gconv2111-{2,7,12,18,25,28}
  gconv             backward arm: dw                                   gconv2111-{3,10,24}
  gconv             backward arm: dbias                                gconv2111-{6,21,31}
  gconv             backward arm: dx-acc+dw                            gconv2111-{5,9,19}
  gconv             backward arm: none                                 gconv2111-{32,33,34,35,36,37}
  gconv             wgrad: S = 1                                       gconv2111-{3,8,9,10,11,13,14,15,17,19,20,21,24,27,30}
  gconv             wgrad: S > 1, rows_per_slice % 4 != 0              gconv2111-{0,1,4,6,16,22,23,26,29,31,38,39}
  gconv             wgrad: S bounded by the thread count               gconv2111-{38,39,40}
  gconv             wgrad: threads % 256 != 0                          gconv2111-{0,1,3,4,5,6,8,9,10,11,14,15,16,17,19,20,21,22,23,24,26,27,29,30,31,39}
  gconv             inputs: ordinary                                   gconv2111-{0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,32,33,34,35,36,37,38,39,40}
  gconv             inputs: corner                                     gconv2111-{26,27,28}
  gconv             inputs: lastpixel                                  gconv2111-{29,30,31}
  conv              64x64 G1, vec epilogue                             conv2212-{0,2,4,5,77,78,81,110,112,113}
  conv              64x64 G1, scalar epilogue                          conv2212-{1,3,67,79,80,118,121}
  conv              64x64 G2, vec epilogue                             conv2212-{6,8,82}
  conv              64x64 G2, scalar epilogue                          conv2212-{7,9,83}
  conv              64x64 G4, vec epilogue                             conv2212-{10,12,84,111}
  conv              64x64 G4, scalar epilogue                          conv2212-{11,13,85}
  conv              128x64, vec epilogue                               conv2212-{14,16,86,88,120}
  conv              128x64, scalar epilogue                            conv2212-{15,17,87}
  conv              128x128 G1, vec epilogue                           conv2212-{18,20,89,91,115,119}
  conv              128x128 G1, scalar epilogue                        conv2212-{19,21,90,122}
  conv              128x128 G2, vec epilogue                           conv2212-{22,24,92}
  conv              128x128 G2, scalar epilogue                        conv2212-{23,25,93}
  conv              256x32, vec epilogue                               conv2212-{26,29,31,33,94,97}
  conv              256x32, scalar epilogue                            conv2212-{27,28,30,32,95,96,117}
  conv              xk, vec epilogue                                   conv2212-{34,35,36,37,38,39,98,99,100,116}
  conv              s2, vec epilogue                                   conv2212-{40,41,42,43,44,45,46,47}
  conv              8p, 8p epilogue                                    conv2212-{54,55,56,57,58,59,60,61,62,63,64,65,66,101,102,103,104,105,106,107,108,109,114}
  conv              pair, vec epilogue                                 conv2212-{48,49,50,51,52,53}
  conv              thin, thin epilogue                                conv2212-{68,69,70,71,72,73,74,75,76,123,124}
  conv              64x64 G1: backward with mask                       conv2212-{0,1,2,5,67,77,121}
  conv              64x64 G1: backward with stats                      conv2212-{0,1,2,67,77}
  conv              64x64 G1: backward with stat_x                     conv2212-{0,1,67}
  conv              64x64 G1: backward with addend                     conv2212-{0,1,67}
  conv              64x64 G1: backward with accumulate                 conv2212-{2,3,77}
  conv              64x64 G2: backward with mask                       conv2212-{6,7,8}
  conv              64x64 G2: backward with stats                      conv2212-{6,7,8}
  conv              64x64 G2: backward with stat_x                     conv2212-{6,7}
  conv              64x64 G2: backward with addend                     conv2212-{6,7}
  conv              64x64 G2: backward with accumulate                 conv2212-{8,9}
  conv              64x64 G4: backward with mask                       conv2212-{10,11,12}
  conv              64x64 G4: backward with stats                      conv2212-{10,11,12,13}
  conv              64x64 G4: backward with stat_x                     conv2212-{10,11}
  conv              64x64 G4: backward with addend                     conv2212-{10,11}
  conv              64x64 G4: backward with accumulate                 conv2212-{12,13}
  conv              128x64: backward with mask                         conv2212-{14,15,16,120}
  conv              128x64: backward with stats                        conv2212-{14,15,16}
  conv              128x64: backward with stat_x                       conv2212-{14,15}
  conv              128x64: backward with addend                       conv2212-{14,15}
  conv              128x64: backward with accumulate                   conv2212-{16,17}
  conv              128x128 G1: backward with mask                     conv2212-{18,19,20,122}
  conv              128x128 G1: backward with stats                    conv2212-{18,19,20}
  conv              128x128 G1: backward with stat_x                   conv2212-{18,19}
  conv              128x128 G1: backward with addend                   conv2212-{18,19}
  conv              128x128 G1: backward with accumulate               conv2212-{20,21}
  conv              128x128 G2: backward with mask                     conv2212-{22,23,24}
  conv              128x128 G2: backward with stats                    conv2212-{22,23,24,25}
  conv              128x128 G2: backward with stat_x                   conv2212-{22,23}
  conv              128x128 G2: backward with addend                   conv2212-{22,23}
  conv              128x128 G2: backward with accumulate               conv2212-{24,25}
  conv              256x32: backward with mask                         conv2212-{26,27,28,29,30,31,33}
  conv              256x32: backward with stats                        conv2212-{26,27,28,29,30,31,33}
  conv              256x32: backward with stat_x                       conv2212-{29,30,33}
  conv              256x32: backward with addend                       conv2212-{29,30,33}
  conv              256x32: backward with accumulate                   conv2212-{31,32}
  conv              xk: backward with mask                             conv2212-{34,35,37,39}
  conv              xk: backward with stats                            conv2212-{34,35,37,39}
  conv              xk: backward with stat_x                           conv2212-{34,35,39}
  conv              xk: backward with addend                           conv2212-{34,36,39}
  conv              xk: backward with accumulate                       conv2212-{37,38}
  conv              s2: backward with mask                             conv2212-{40,41,42,43,47}
  conv              s2: backward with stats                            conv2212-{40,41,43,46,47}
  conv              s2: backward with stat_x                           conv2212-{40,41,47}
  conv              s2: backward with addend                           conv2212-{40,44,47}
  conv              s2: backward with accumulate                       conv2212-{43,45}
  conv              8p: backward with mask                             conv2212-{55,56,59,61,62,63,64,65,66}
  conv              8p: backward with stats                            conv2212-{55,56,58,61,62,64,65,66}
  conv              8p: backward with stat_x                           conv2212-{55,56,64,65}
  conv              8p: backward with addend                           conv2212-{56,60,64}
  conv              8p: backward with accumulate                       conv2212-{57,61,66}
  conv              pair: backward with mask                           conv2212-{48,49,50,51,52}
  conv              pair: backward with stats                          conv2212-{48,49,50,51,52}
  conv              pair: backward with stat_x                         conv2212-{50,51}
  conv              pair: backward with addend                         conv2212-{50,51}
  conv              pair: backward with accumulate                     conv2212-{52,53}
  conv              thin: backward with mask                           conv2212-{72,73,74,75,76,123,124}
  conv              thin: backward with stats                          conv2212-{69,71,73,75,123}
  conv              thin: backward with accumulate                     conv2212-{70,71}
  conv              64x64 G1: forward                                  conv2212-{78,79,80,81,110,112,113,118}
  conv              64x64 G2: forward                                  conv2212-{82,83}
  conv              64x64 G4: forward                                  conv2212-{84,85,111}
  conv              128x64: forward                                    conv2212-{86,87,88}
  conv              128x128 G1: forward                                conv2212-{89,90,91,115,119}
  conv              128x128 G2: forward                                conv2212-{92,93}
  conv              256x32: forward                                    conv2212-{94,95,96,97,117}
  conv              xk: forward                                        conv2212-{98,99,100,116}
  conv              8p: forward                                        conv2212-{101,102,103,104,105,106,107,108,109,114}
  conv              vec epilogue, forward with bias                    conv2212-{78,84,86,89,91,92,98,100,110,113,116}
  conv              vec epilogue, forward with scale                   conv2212-{84,92,100,113}
  conv              vec epilogue, forward with residual                conv2212-{78,89,98,112}
  conv              vec epilogue, forward with relu                    conv2212-{78,82,84,88,89,94,97,98,99,100,115}
  conv              vec epilogue, forward with stats                   conv2212-{82,94,99}
  conv              vec epilogue, forward with out_f32                 conv2212-{86,119}
  conv              scalar epilogue, forward with bias                 conv2212-{79,80,87,95,96,118}
  conv              scalar epilogue, forward with scale                conv2212-{79,87}
  conv              scalar epilogue, forward with residual             conv2212-{80,83}
  conv              scalar epilogue, forward with relu                 conv2212-{79,80,90}
  conv              scalar epilogue, forward with stats                conv2212-{85,90}
  conv              scalar epilogue, forward with out_f32              conv2212-{93,96,117,118}
  conv              8p epilogue, forward with bias                     conv2212-{102,103,105,106,114}
  conv              8p epilogue, forward with scale                    conv2212-{103,106}
  conv              8p epilogue, forward with residual                 conv2212-{102,107,114}
  conv              8p epilogue, forward with relu                     conv2212-{102,103,104,109,114}
  conv              8p epilogue, forward with stats                    conv2212-{104,108}
  conv              8p epilogue, forward with out_f32                  conv2212-{101,105}
  conv              vec epilogue, backward with mask                   conv2212-{0,2,5,6,8,10,12,14,16,18,20,22,24,26,29,31,33,34,35,37,39,40,41,42,43,47,48,49,50,51,52,77,120}
  conv              vec epilogue, backward with stats                  conv2212-{0,2,6,8,10,12,14,16,18,20,22,24,26,29,31,33,34,35,37,39,40,41,43,46,47,48,49,50,51,52,77}
  conv              vec epilogue, backward with stat_x                 conv2212-{0,6,10,14,18,22,29,33,34,35,39,40,41,47,50,51}
  conv              vec epilogue, backward with addend                 conv2212-{0,6,10,14,18,22,29,33,34,36,39,40,44,47,50,51}
  conv              vec epilogue, backward with accumulate             conv2212-{2,8,12,16,20,24,31,37,38,43,45,52,53,77}
  conv              vec epilogue, backward with mask_scale             conv2212-{42,120}
  conv              scalar epilogue, backward with mask                conv2212-{1,7,11,15,19,23,27,28,30,67,121,122}
  conv              scalar epilogue, backward with stats               conv2212-{1,7,11,13,15,19,23,25,27,28,30,67}
  conv              scalar epilogue, backward with stat_x              conv2212-{1,7,11,15,19,23,30,67}
  conv              scalar epilogue, backward with addend              conv2212-{1,7,11,15,19,23,30,67}
  conv              scalar epilogue, backward with accumulate          conv2212-{3,9,13,17,21,25,32}
  conv              scalar epilogue, backward with mask_scale          conv2212-{121,122}
  conv              64x64 G1: ragged last M tile                       conv2212-{0,1,2,3,4,5,67,77,78,79,80,81,110,112,113,118,121}
  conv              64x64 G2: ragged last M tile                       conv2212-{6,7,8,9,82,83}
  conv              64x64 G4: ragged last M tile                       conv2212-{10,11,12,13,84,85,111}
  conv              128x64: ragged last M tile                         conv2212-{14,15,16,17,86,87,88,120}
  conv              128x128 G1: ragged last M tile                     conv2212-{18,19,20,21,89,90,91,115,119,122}
  conv              128x128 G2: ragged last M tile                     conv2212-{22,23,24,25,92,93}
  conv              256x32: ragged last M tile                         conv2212-{26,27,28,29,30,31,32,33,94,95,96,97,117}
  conv              xk: ragged last M tile                             conv2212-{34,35,36,37,38,39,98,99,100,116}
  conv              8p: ragged last M tile                             conv2212-{54,55,56,57,58,59,60,61,62,63,64,65,66,101,102,103,104,105,106,107,108,109,114}
  conv              pair: ragged last M tile                           conv2212-{48,49,50,51,52,53}
  conv              64x64 G1: ragged last OC tile                      conv2212-{0,1,2,3,4,5,67,78,79,80,81,110,112,113,118,121}
  conv              64x64 G2: ragged last OC tile                      conv2212-{6,7,8,9,82,83}
  conv              64x64 G4: ragged last OC tile                      conv2212-{10,11,12,13,84,85,111}
  conv              128x64: ragged last OC tile                        conv2212-{14,15,16,17,86,87,88,120}
  conv              128x128 G1: ragged last OC tile                    conv2212-{18,19,20,21,89,90,91,115,119,122}
  conv              128x128 G2: ragged last OC tile                    conv2212-{22,23,24,25,92,93}
  conv              256x32: ragged last OC tile                        conv2212-{26,27,28,29,30,31,32,33,94,95,96,97,117}
  conv              xk: ragged last OC tile                            conv2212-{34,35,36,37,38,39,98,99,100,116}
  conv              s2: ragged last OC tile                            conv2212-{40,42,44,46}
  conv              8p: ragged last OC tile                            conv2212-{54,55,56,57,58,59,60,61,62,63,64,65,66,101,102,103,104,105,106,107,108,109,114}
  conv              pair: ragged last OC tile                          conv2212-{48,49,50,51,52,53}
  conv              scalar epilogue by alignment alone, fwd            conv2212-{83,85,93}
  conv              scalar epilogue by alignment alone, bwd            conv2212-{1,7,9,11,15,21,23,67}
  conv              in view: ld                                        conv2212-{79,96}
  conv              in view: bs                                        conv2212-{84,116}
  conv              in view: ld+bs                                     conv2212-{81,88,103}
  conv              out view: ld                                       conv2212-{82,85,86,93,94,98,105,113}
  conv              out view: bs                                       conv2212-{78,92,100}
  conv              out view: ld+bs                                    conv2212-{91,102,108}
  conv              res view: ld                                       conv2212-{78,83,102,114}
  conv              res view: bs                                       conv2212-{80,107}
  conv              res view: ld+bs                                    conv2212-{89,98}
  conv              x view: ld                                         conv2212-{1,20,69,124}
  conv              x view: bs                                         conv2212-{8,15,72}
  conv              x view: ld+bs                                      conv2212-{3,11}
  conv              dy view: ld                                        conv2212-{2,11,20}
  conv              dy view: bs                                        conv2212-{1,8}
  conv              dy view: ld+bs                                     conv2212-{15,24}
  conv              dx view: ld                                        conv2212-{1,9,14,36,43,53,57}
  conv              dx view: bs                                        conv2212-{13,38,50}
  conv              dx view: ld+bs                                     conv2212-{2,21,31,40,66,70}
  conv              mask view: ld                                      conv2212-{0,1,16,23,26,34,40,48,55,62,67,74}
  conv              mask view: bs                                      conv2212-{5,18,28,41,59,76,122}
  conv              mask view: ld+bs                                   conv2212-{10,15,42,56,64,75}
  conv              statx view: ld                                     conv2212-{6,11,41,64}
  conv              statx view: bs                                     conv2212-{10,55}
  conv              statx view: ld+bs                                  conv2212-{22,35,47,65}
  conv              addend view: ld                                    conv2212-{7,18,29,44,56}
  conv              addend view: bs                                    conv2212-{0,47,64}
  conv              addend view: ld+bs                                 conv2212-{6,36,50,60}
  conv              fwd, f32                                           conv2212-{79,83,88,90,91,96,97,111}
  conv              fwd, bf16                                          conv2212-{78,80,81,82,84,85,86,87,89,92,93,94,95,98,99,100,101,102,103,104,105,106,107,108,109,110,112,119}
  conv              fwd, f16                                           conv2212-{113,114,115,116,117,118}
  conv              bwd, f32                                           conv2212-{1,8,9,12,13,15,20,21,28,29,32,43,45,46,49,51,53,69,73,74,122}
  conv              bwd, bf16                                          conv2212-{0,2,3,4,5,6,7,10,11,14,16,17,18,19,22,23,24,25,26,27,30,31,33,34,35,36,37,38,39,40,41,42,44,47,48,50,52,54,55,56,57,58,59,60,61,62,63,64,65,66,67,68,70,71,72,75,76,77,120,121,123,124}
  conv              forward epilogue: none                             conv2212-{81,111}
  conv              forward epilogue: bias                             conv2212-{91,95,110,116}
  conv              forward epilogue: fold                             conv2212-{87,92,106,113}
  conv              forward epilogue: residual                         conv2212-{83,107,112}
  conv              forward epilogue: relu                             conv2212-{88,97,109,115}
  conv              forward epilogue: stats                            conv2212-{85,108}
  conv              forward epilogue: out_f32                          conv2212-{93,101,117,119}
  conv              forward epilogue: bias+residual+relu               conv2212-{78,80,89,98,102,114}
  conv              forward epilogue: fold+relu                        conv2212-{79,84,100,103}
  conv              forward epilogue: stats+relu                       conv2212-{82,90,94,99,104}
  conv              forward epilogue: out_f32+bias                     conv2212-{86,96,105,118}
  conv              backward epilogue: none                            conv2212-{4,54,68}
  conv              backward epilogue: stats                           conv2212-{46,58,69}
  conv              backward epilogue: mask                            conv2212-{5,59,74}
  conv              backward epilogue: mask+stats                      conv2212-{26,27,28,48,49,62,75}
  conv              backward epilogue: mask+stats+stat_x               conv2212-{35,41,55,65}
  conv              backward epilogue: mask+scale                      conv2212-{42,63,76,120,121,122}
  conv              backward epilogue: addend                          conv2212-{36,44,60}
  conv              backward epilogue: addend+mask+stats+stat_x        conv2212-{0,1,6,7,10,11,14,15,18,19,22,23,29,30,33,34,39,40,47,50,51,56,64,67}
  conv              backward epilogue: accumulate                      conv2212-{3,9,17,21,32,38,45,53,57,70}
  conv              backward epilogue: accumulate+mask+stats           conv2212-{2,8,12,16,20,24,31,37,43,52,61,66,77}
  conv              backward epilogue: accumulate+stats                conv2212-{13,25,71}
  conv              backward epilogue: maskx                           conv2212-{72,124}
  conv              backward epilogue: maskx+stats                     conv2212-{73,123}
  conv              backward arm: dx                                   conv2212-{0,2,4,5,6,7,9,10,12,13,14,16,17,18,19,21,22,24,25,28,29,30,31,32,33,34,36,37,38,39,40,42,43,44,45,46,47,54,55,57,58,59,60,62,63,64,65,66,67,120,121,122}
  conv              backward arm: dx+dw                                conv2212-{1,8,11,20,23,26,35,41,50,52,56,69,71,73,74,76,77,124}
  conv              backward arm: dx+dw+dbias                          conv2212-{3,15,27,48,49,51,53,61,68,70,72,75,123}
  conv              xk = 2 asked                                       conv2212-{34,38,98,116}
  conv              xk = 3 asked                                       conv2212-{35,39,99}
  conv              xk = 8 asked                                       conv2212-{36,37,100}
  conv              xk: fewer k-tiles than the copies asked for        conv2212-{37,39,100}
  conv              8p: k = 3, tap-major                               conv2212-{54,55,56,57,101,102,107,109,114}
  conv              8p: k = 3, channel-block-major                     conv2212-{58,59,60,61,103}
  conv              8p: k = 1, tap-major                               conv2212-{62,63,64,105,106,108}
  conv              8p: k = 1, channel-block-major                     conv2212-{65,66,104}
  conv              8p asked, refused by igemm8p_ok: the ladder's kernel conv2212-{67}
  conv              s2: k = 3 pad 1                                    conv2212-{40,41,46,47}
  conv              s2: k = 5 pad 2                                    conv2212-{42,43}
  conv              s2: k = 2 pad 0                                    conv2212-{44,45}
  conv              s2: 1 x 16 x 16                                    conv2212-{40,42,44,46}
  conv              s2: 2 x 8 x 16                                     conv2212-{41,43,45,47}
  conv              s2: generic twin, bit-identical dx                 conv2212-{40,41,42,43,44,45,46,47}
  conv              thin: MASK 0                                       conv2212-{68,69,70,71}
  conv              thin: MASK 1 (mask_y is x)                         conv2212-{72,73,123,124}
  conv              thin: MASK 2                                       conv2212-{74,75,76}
  conv              thin: 4 channels per thread                        conv2212-{68,74,123}
  conv              thin: 8 channels per thread                        conv2212-{69,70,71,72,73,75,76,124}
  conv              thin: generic twin                                 conv2212-{68,69,70,71,72,73,74,75,76,123,124}
  conv              thin shape refused by thin_bwd_ok                  conv2212-{77}
  conv              grouped launch: emrt_conv2d_dgrad_multi            conv2212-{125,126,127}
  conv              grouped launch: emrt_conv2d_group                  conv2212-{128,129,130}
  conv              inputs: ordinary                                   conv2212-{0,1,2,3,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31,32,33,34,35,36,37,38,39,40,41,42,43,44,45,46,48,49,50,51,52,54,55,56,57,58,60,61,62,63,64,65,67,68,69,70,71,72,73,74,75,77,78,79,80,82,83,84,85,86,87,88,89,90,92,93,94,95,96,97,98,99,100,101,102,103,104,105,107,108,109,110,111,112,113,114,115,116,117,118,119,120,121,122,123,124}
  conv              inputs: corner                                     conv2212-{4,53,59,81}
  conv              inputs: lastpixel                                  conv2212-{5,47,66,76,91,106}
  loss              family: ce                                         loss-{0,1,2,3,4,5,6,7,8,9,10,11,12,13,14}
  loss              family: wce                                        loss-{15,16,17,18,19,20,21,22,23,24,25,26,27,28}
  loss              family: ohem                                       loss-{29,30,31,32,33,34,35,36,37,38,39,40,41,42,43,44}
  loss              family: dice                                       loss-{45,46,47,48,49,50,51,52,53,54,55,56}
  loss              form: single                                       loss-{0,2,4,6,8,10,11,13,14,15,17,19,21,23,25,27,29,31,33,35,37,38,40,41,43,45,47,49,51,53,54,55}
  loss              form: pair                                         loss-{1,3,5,7,9,12,16,18,20,22,24,26,28,30,32,34,36,39,42,44,46,48,50,52,56}
  loss              C = 1                                              loss-{0,15,45}
  loss              C = 2                                              loss-{1,14,16,28,29,42,44,46,56}
  loss              C = 3                                              loss-{2,17,30,41,43,47}
  loss              C = 6                                              loss-{3,5,13,18,27,31,34,40,54,55}
  loss              C = 7                                              loss-{4,19,20,32,50}
  loss              C = 8                                              loss-{6,21,33,48}
  loss              C = 9                                              loss-{7,22,35,49}
  loss              C = 16                                             loss-{8,23,36,51}
  loss              C = 17                                             loss-{9,24,37,52}
  loss              C = 19                                             loss-{10,25,38,53}
  loss              C = 150                                            loss-{11,12,26,39}
  loss              dice: whole class chunks (C % 8 == 0)              loss-{48,51}
  loss              dice: several chunks, ragged last                  loss-{49,52,53}
  loss              1 pixel                                            loss-{0,15,29,45}
  loss              15 pixels                                          loss-{1,16,30,46}
  loss              255 pixels                                         loss-{2,6,17,21,31,36,47,51}
  loss              256 pixels                                         loss-{3,18,32,48}
  loss              257 pixels                                         loss-{4,19,33,49}
  loss              a block spans two images (N >= 2, HW % 256 != 0)   loss-{5,7,20,23,34,35,41,42,50,55}
  loss              several images inside one block                    loss-{6,8,12,13,21,22,27,36,37,40,51,52,54}
  loss              ce: the forward grid strides                       loss-{14}
  loss              wce: the forward grid strides                      loss-{28}
  loss              ohem: the forward grid strides                     loss-{44}
  loss              dice: the forward grid strides                     loss-{56}
  loss              ohem: the digit histograms' grid strides           loss-{43,44}
  loss              second trip: wce_bwd_kernel plain, single          loss-{14}
  loss              second trip: wce_bwd_kernel weighted, pair         loss-{28}
  loss              second trip: ohem_bwd_kernel                       loss-{44}
  loss              second trip: dice_bwd_kernel                       loss-{56}
  loss              labels: none                                       loss-{0,2,9,15,18,25,29,32,45,48}
  loss              labels: tenth                                      loss-{1,3,5,6,7,8,11,12,14,16,17,19,20,21,23,26,28,30,31,34,35,36,37,39,41,42,43,44,46,47,49,50,51,55,56}
  loss              labels: all                                        loss-{13,27,40,54}
  loss              labels: allbut1                                    loss-{4,22,33,52}
  loss              labels: oneclass                                   loss-{10,24,38,53}
  loss              ignore index 255                                   loss-{0,1,2,4,5,7,8,10,11,13,14,15,16,18,19,20,22,23,24,26,27,28,29,30,32,33,34,36,37,38,39,40,41,42,43,44,45,46,48,49,50,52,53,54,55,56}
  loss              ignore index -100                                  loss-{3,9,17,25,31,47}
  loss              ignore index inside [0, C)                         loss-{6,12,21,35,51}
  loss              logits: ordinary                                   loss-{0,1,2,4,5,10,11,13,14,15,16,18,19,20,26,27,28,29,30,31,33,34,39,40,43,45,46,48,49,50,54,56}
  loss              logits: confident                                  loss-{3,17,25,32,35,47}
  loss              logits: shift+                                     loss-{6,22,36,51}
  loss              logits: shift-                                     loss-{7,21,38,55}
  loss              logits: wide                                       loss-{8,12,23,37,52}
  loss              logits: constant                                   loss-{9,24,41,53}
  loss              logits: grid                                       loss-{42,44}
  loss              class weights: random                              loss-{15,16,18,20,21,22,23,25,26,27,28,47,50,54}
  loss              class weights: onezero                             loss-{17,24,52}
  loss              class weights: zeropresent                         loss-{19,55}
  loss              head weights (1, 0.4)                              loss-{0,1,2,4,5,6,8,9,10,11,13,14,15,16,17,19,20,21,23,24,25,26,27,28,29,30,31,33,34,35,37,38,39,40,41,42,43,44,45,46,47,49,50,51,53,54,55,56}
  loss              one negative head weight                           loss-{3,12,22,32,48}
  loss              one head weight zero                               loss-{7,18,36,52}
  loss              upstream scalar given                              loss-{1,5,10,12,18,20,23,28,32,34,38,44,48,50}
  loss              upstream NULL                                      loss-{0,2,3,4,6,7,8,9,11,13,14,15,16,17,19,21,22,24,25,26,27,29,30,31,33,35,36,37,39,40,41,42,43,45,46,47,49,51,52,53,54,55,56}
  loss              ohem: min_kept = 0                                 loss-{29,40}
  loss              dice: smooth 0                                     loss-{48,49}
  step              entry: clip                                        step-{0,1,2,3,4,5,6,7,8,9,10,11}
  step              entry: sgd                                         step-{12,13,14,15,16,17,18,19,20,21,22,23,24,25}
  step              entry: sgd_sched                                   step-{26,27,28}
  step              entry: adamw                                       step-{29,30,31,32,33,34,35,36,37,38,39}
  step              n = 1                                              step-{0,12,29}
  step              n = 3                                              step-{1,10,13,30}
  step              n = 4                                              step-{2,14,31}
  step              n = 5                                              step-{3,15,28,32}
  step              1023 quads                                         step-{4,7,9,16,17,22,33,37}
  step              1024 quads                                         step-{5,8,18,19,24,26,27,34}
  step              1025 quads                                         step-{6,20,21,23,35,36,38}
  step              tail of 0                                          step-{2,4,8,14,16,20,24,31,34,36}
  step              tail of 1                                          step-{0,3,5,12,15,17,23,27,28,29,32,37,38}
  step              tail of 2                                          step-{6,9,18,22,35}
  step              tail of 3                                          step-{1,7,10,11,13,19,21,25,26,30,33,39}
  step              clip: the partial sums' grid strides               step-{11}
  step              sgd: stream_update's grid strides                  step-{25}
  step              adamw: stream_update's grid strides                step-{39}
  step              ranges: none                                       step-{12,29}
  step              ranges: whole                                      step-{13,14,27,30}
  step              ranges: quad16                                     step-{16,17,26,33}
  step              ranges: inquad                                     step-{18,31}
  step              ranges: intail                                     step-{15,21,32,39}
  step              ranges: border                                     step-{19,25,35}
  step              ranges: r32                                        step-{20,34}
  step              ranges: adjacent                                   step-{22,36}
  step              ranges: empty                                      step-{23,37}
  step              ranges: past                                       step-{24,28,38}
  step              mirror: none                                       step-{12,15,17,20,24,27,29,31,34,37}
  step              mirror: bf16                                       step-{13,16,19,21,23,25,26,30,33,36,38}
  step              mirror: fp16                                       step-{14,18,22,28,32,35,39}
  step              sgd_nt = 0                                         step-{13,17,21,22,27,31,34,38}
  step              sgd_nt = 1                                         step-{12,14,15,16,18,19,20,23,24,25,26,28,29,30,32,33,35,36,37,39}
  step              clip kind: below                                   step-{1,6}
  step              clip kind: above                                   step-{0,5,7,11}
  step              clip kind: zero                                    step-{2,8}
  step              clip kind: negative                                step-{3,9}
  step              clip kind: zerograd                                step-{4,10}
  step              step NULL                                          step-{22,27,37}
  step              clip_state NULL                                    step-{19,27,35}
  step              lr_out NULL                                        step-{14,27,36}
  areas             1 class                                            areas-{0,1}
  areas             2 classes                                          areas-{2,3}
  areas             19 classes                                         areas-{4,5,6,10}
  areas             256 classes                                        areas-{7,8,9}
  areas             labels: int32                                      areas-{0,4,7}
  areas             labels: int64                                      areas-{1,5,8}
  areas             labels: uint8                                      areas-{2,3,6,9,10}
  areas             uint8 at byte offset 0                             areas-{2,9}
  areas             uint8 at byte offset 1                             areas-{3,6,10}
  areas             n = 1                                              areas-{0,8}
  areas             n = 4095                                           areas-{1,5,9}
  areas             n = 4096                                           areas-{2,6,7}
  areas             n = 4097                                           areas-{3,4}
  areas             the grid strides (n > 1024 x 4096)                 areas-{10}
  areas             ignore index inside [0, ncls)                      areas-{1,3,8,9}
  areas             ignore index outside [0, ncls)                     areas-{0,2,4,5,6,7,10}
  dropout           element mode                                       drop-{0,1,2,3,4,5,6,7,8,9,10,11}
  dropout           channel mode                                       drop-{12,13,14,15,16,17,18,19,20}
  dropout           element: n = 4                                     drop-{0,1}
  dropout           element: n = 1020                                  drop-{2,3,4}
  dropout           element: n = 1024                                  drop-{5,6,7}
  dropout           element: n = 1028                                  drop-{8,9,10}
  dropout           element: the second trip (n > 8192 x 1024)         drop-{11}
  dropout           channel: N > 1, hw = 1                             drop-{12,13,14}
  dropout           channel: N > 1, hw = 25                            drop-{15,16,17,18}
  dropout           channel: C = 4                                     drop-{12,15}
  dropout           channel: C = 64                                    drop-{13,16,19,20}
  dropout           channel: C = 100                                   drop-{14,17,18}
  dropout           channel: C hw % 1024 != 0                          drop-{12,13,14,15,16,17,18}
  dropout           p = 0                                              drop-{0,5,19}
  dropout           p = 2^-17 (threshold 0)                            drop-{2,8,14}
  dropout           p = 0.1                                            drop-{3,6,13,17}
  dropout           p = 0.5                                            drop-{1,7,9,11,12,15,16,20}
  dropout           p = 0.999                                          drop-{4,10,18}
  dropout           backward arm: mask                                 drop-{1,2,4,6,7,9,11,12,14,15,16,17,18}
  dropout           backward arm: mask+relu                            drop-{3,6,8,9,10,13,15,17,20}
  dropout           backward arm: relu                                 drop-{0,5,19}
  dropout           backward arm: stored                               drop-{1,4,6,8}
  dropout           channel mode, backward with relu_out               drop-{13,15,17,20}
  dropout           seed 0                                             drop-{2,7,12,17}
  dropout           seed with the top bit set                          drop-{3,8,13,18}
  dropout           salt 0                                             drop-{7,15}
  layernorm_drop    C = 12                                             lnd-{0,1}
  layernorm_drop    C = 100                                            lnd-{2,3}
  layernorm_drop    C = 256                                            lnd-{4,5,6,7}
  layernorm_drop    C = 260                                            lnd-{8,9,10}
  layernorm_drop    C = 1000                                           lnd-{11,12,13}
  layernorm_drop    C = 1024                                           lnd-{14,15,16}
  layernorm_drop    rows % 4 != 0                                      lnd-{0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16}
  layernorm_drop    rows = 1                                           lnd-{0,3,10,13}
  layernorm_drop    form ln(a+b)                                       lnd-{0,4,8,13,15}
  layernorm_drop    form ln(a+b,post)                                  lnd-{1,5,11,16}
  layernorm_drop    form ln(a+b,qpos)                                  lnd-{2,6,10,12}
  layernorm_drop    form ln(a+b,addend)                                lnd-{3,7,9,14}
  layernorm_drop    p = 0.1                                            lnd-{1,3,4,6,9,11,13,15}
  layernorm_drop    p = 0.5                                            lnd-{0,2,5,7,8,10,12,14,16}
  layernorm_drop    backward under the default knobs                   lnd-{0,1,2,3,4,8,10,11,13,14}
  layernorm_drop    backward under ln_bwd_rows                         lnd-{6,7,9,12,16}
  layernorm_drop    backward under ln_bwd_max_blocks                   lnd-{5,6,12,15}
  layernorm_drop    backward blocks loop under the block cap           lnd-{5,6,12,15}
  layernorm_drop    several backward blocks                            lnd-{2,4,5,6,7,8,9,11,12,14,15,16}
  conv_drop         M = 1                                              cdrop-{0,1}
  conv_drop         M = 63                                             cdrop-{2,3}
  conv_drop         M = 64                                             cdrop-{4,5,11}
  conv_drop         M = 65                                             cdrop-{6,7}
  conv_drop         M = 114                                            cdrop-{8,9,10}
  conv_drop         C = 8                                              cdrop-{0,2,5,10}
  conv_drop         C = 64                                             cdrop-{1,4,6,8}
  conv_drop         C = 264                                            cdrop-{3,7,9,11}
  conv_drop         OC = 8                                             cdrop-{0,4,7}
  conv_drop         OC = 72                                            cdrop-{1,3,8,11}
  conv_drop         OC = 96                                            cdrop-{2,6,10}
  conv_drop         OC = 1024                                          cdrop-{5,9}
  conv_drop         ldout == OC                                        cdrop-{0,1,2,4,5,6,8,11}
  conv_drop         ldout > OC (a slice of a wider buffer)             cdrop-{3,7,9,10}
  conv_drop         ldin > C                                           cdrop-{5,8}
  conv_drop         ragged last M tile                                 cdrop-{0,1,2,3,6,7,8,9,10}
  conv_drop         several M tiles                                    cdrop-{6,7,8,9,10}
  conv_drop         several N tiles                                    cdrop-{1,2,3,5,6,8,9,10,11}
  conv_drop         ragged last N tile                                 cdrop-{0,1,2,3,4,6,7,8,10,11}
  conv_drop         p = 0.1                                            cdrop-{1,3,5,6,9,11}
  conv_drop         p = 0.5                                            cdrop-{0,2,4,7,8,10}
  elementwise       kernel: add, f32                                   ew-{0,3,6,9,12,15,18,21,24,27,30}
  elementwise       kernel: add, bf16                                  ew-{1,4,7,10,13,16,19,22,25,28,31,33}
  elementwise       kernel: add, f16                                   ew-{2,5,8,11,14,17,20,23,26,29,32}
  elementwise       kernel: add_f32row, f32                            ew-{34,37,40,43,46,49,52,55,58,61,64}
  elementwise       kernel: add_f32row, bf16                           ew-{35,38,41,44,47,50,53,56,59,62,65,67}
  elementwise       kernel: add_f32row, f16                            ew-{36,39,42,45,48,51,54,57,60,63,66}
  elementwise       kernel: levels, f32                                ew-{68,71,74,77,80,83,86,89,92,95,98}
  elementwise       kernel: levels, bf16                               ew-{69,72,75,78,81,84,87,90,93,96,99,101}
  elementwise       kernel: levels, f16                                ew-{70,73,76,79,82,85,88,91,94,97,100}
  elementwise       kernel: add3d, f32                                 ew-{102,105,108,111,114,117,120,123,126,129,132,135,138,141}
  elementwise       kernel: add3d, bf16                                ew-{103,106,109,112,115,118,121,124,127,130,133,136,139,142,144}
  elementwise       kernel: add3d, f16                                 ew-{104,107,110,113,116,119,122,125,128,131,134,137,140,143}
  elementwise       kernel: acc3d, f32                                 ew-{145,148,151,154,157,160,163,166,169,172,175,178}
  elementwise       kernel: acc3d, bf16                                ew-{146,149,152,155,158,161,164,167,170,173,176,179,181}
  elementwise       kernel: acc3d, f16                                 ew-{147,150,153,156,159,162,165,168,171,174,177,180}
  elementwise       kernel: concat, f32                                ew-{182,185,188,191,194,197,200,203,206,209}
  elementwise       kernel: concat, bf16                               ew-{183,186,189,192,195,198,201,204,207,210,212}
  elementwise       kernel: concat, f16                                ew-{184,187,190,193,196,199,202,205,208,211}
  elementwise       kernel: split, f32                                 ew-{213,216,219,222,225,228,231,234,237,240}
  elementwise       kernel: split, bf16                                ew-{214,217,220,223,226,229,232,235,238,241,243}
  elementwise       kernel: split, f16                                 ew-{215,218,221,224,227,230,233,236,239,242}
  elementwise       kernel: cast_to, bf16                              ew-{244,245,246,247}
  elementwise       kernel: cast_to, f16                               ew-{248,249,250,251,252}
  elementwise       kernel: cast_from, bf16                            ew-{253,254,255,256,261}
  elementwise       kernel: cast_from, f16                             ew-{257,258,259,260}
  elementwise       kernel: sigmoid_fwd, f32                           ew-{262,263,264,265}
  elementwise       kernel: sigmoid_bwd, f32                           ew-{266,267,268,269}
  elementwise       kernel: memcpy, f32                                ew-{270,271,272,273,274,275,276}
  elementwise       second trip: add                                   ew-{33}
  elementwise       second trip: add_f32row                            ew-{67}
  elementwise       second trip: levels                                ew-{101}
  elementwise       second trip: add3d                                 ew-{144}
  elementwise       second trip: acc3d                                 ew-{181}
  elementwise       second trip: concat                                ew-{212}
  elementwise       second trip: split                                 ew-{243}
  elementwise       second trip: cast_to                               ew-{252}
  elementwise       second trip: cast_from                             ew-{261}
  elementwise       second trip: sigmoid_fwd                           ew-{265}
  elementwise       second trip: sigmoid_bwd                           ew-{269}
  elementwise       second trip: memcpy                                ew-{276}
  elementwise       1 lane                                             ew-{0,1,2,34,35,36,68,69,70,102,103,104,145,146,147,182,183,184,213,214,215,244,248,253,257,262,266}
  elementwise       255 lanes                                          ew-{3,4,5,6,7,8,9,10,11,12,13,14,37,38,39,40,41,42,43,44,45,46,47,48,92,93,94,105,106,107,114,115,116,117,118,119,120,121,122,123,124,125,126,127,128,129,130,131,148,149,150,157,158,159,160,161,162,163,164,165,166,167,168,203,204,205,234,235,236,246,250,255,259}
  elementwise       256 lanes                                          ew-{15,16,17,18,19,20,21,22,23,49,50,51,52,53,54,55,56,57,95,96,97,108,109,110,151,152,153,206,207,208,237,238,239}
  elementwise       257 lanes                                          ew-{24,25,26,27,28,29,30,31,32,58,59,60,61,62,63,64,65,66,98,99,100,111,112,113,154,155,156,209,210,211,240,241,242,247,251,256,260,263,267}
  elementwise       add: period == n                                   ew-{0,1,2,3,4,5,15,16,17,24,25,26,34,35,36,37,38,39,49,50,51,58,59,60}
  elementwise       add: period 4                                      ew-{6,7,8,27,28,29,40,41,42,61,62,63}
  elementwise       add: period divides n                              ew-{9,10,11,18,19,20,43,44,45,52,53,54}
  elementwise       add: period does not divide n                      ew-{12,13,14,21,22,23,30,31,32,46,47,48,55,56,57,64,65,66}
  elementwise       levels: L = 1                                      ew-{68,69,70,71,72,73,95,96,97}
  elementwise       levels: L = 2                                      ew-{74,75,76,77,78,79,92,93,94}
  elementwise       levels: L = 3                                      ew-{80,81,82,83,84,85,98,99,100,101}
  elementwise       levels: L = 4                                      ew-{86,87,88,89,90,91}
  elementwise       levels: a level of one row                         ew-{68,69,70,74,75,76,77,78,79,80,81,82,83,84,85,86,87,88,89,90,91,98,99,100,101}
  elementwise       levels: the last level of one row                  ew-{74,75,76,80,81,82,86,87,88,98,99,100}
  elementwise       levels: C = 4                                      ew-{68,69,70,83,84,85,86,87,88,92,93,94,95,96,97,98,99,100,101}
  elementwise       levels: C = 100                                    ew-{71,72,73,74,75,76,89,90,91}
  elementwise       levels: C = 256                                    ew-{77,78,79,80,81,82}
  elementwise       add3d: operand 0 a slab, the others dense          ew-{114,115,116}
  elementwise       add3d: operand 0 a slice, the others dense         ew-{117,118,119}
  elementwise       add3d: operand 1 a slab, the others dense          ew-{120,121,122}
  elementwise       add3d: operand 1 a slice, the others dense         ew-{123,124,125}
  elementwise       add3d: operand 2 a slab, the others dense          ew-{126,127,128}
  elementwise       add3d: operand 2 a slice, the others dense         ew-{129,130,131}
  elementwise       acc3d: operand 0 a slab, the others dense          ew-{157,158,159}
  elementwise       acc3d: operand 0 a slice, the others dense         ew-{160,161,162}
  elementwise       acc3d: operand 1 a slab, the others dense          ew-{163,164,165}
  elementwise       acc3d: operand 1 a slice, the others dense         ew-{166,167,168}
  elementwise       add3d: every operand strided                       ew-{132,133,134,135,136,137,138,139,140,141,142,143}
  elementwise       acc3d: every operand strided                       ew-{169,170,171,172,173,174,175,176,177,178,179,180}
  elementwise       add3d: B = 1                                       ew-{102,103,104,111,112,113,138,139,140}
  elementwise       acc3d: B = 1                                       ew-{145,146,147,154,155,156,175,176,177}
  elementwise       add3d: rows = 1                                    ew-{102,103,104,141,142,143}
  elementwise       acc3d: rows = 1                                    ew-{145,146,147,178,179,180}
  elementwise       concat: 1 part                                     ew-{182,183,184,185,186,187}
  elementwise       concat: 4 parts                                    ew-{188,189,190,191,192,193,194,195,196}
  elementwise       concat: 8 parts                                    ew-{197,198,199,200,201,202}
  elementwise       split: 1 part                                      ew-{213,214,215,216,217,218}
  elementwise       split: 4 parts                                     ew-{219,220,221,222,223,224,225,226,227}
  elementwise       split: 8 parts                                     ew-{228,229,230,231,232,233}
  elementwise       concat / split: a part of one token first          ew-{188,189,190,197,198,199,209,210,211,219,220,221,228,229,230,240,241,242}
  elementwise       concat / split: a part of one token last           ew-{191,192,193,200,201,202,206,207,208,212,222,223,224,231,232,233,237,238,239,243}
  elementwise       concat / split: a part of one token in the middle  ew-{194,195,196,200,201,202,225,226,227,231,232,233}
  elementwise       concat / split: B = 1                              ew-{182,183,184,188,189,190,197,198,199,206,207,208,209,210,211,212,213,214,215,219,220,221,228,229,230,237,238,239,240,241,242,243}
  elementwise       concat / split: B = 3                              ew-{185,186,187,191,192,193,194,195,196,200,201,202,203,204,205,216,217,218,222,223,224,225,226,227,231,232,233,234,235,236}
  elementwise       concat / split: C = 4                              ew-{182,183,184,191,192,193,197,198,199,203,204,205,206,207,208,209,210,211,212,213,214,215,222,223,224,228,229,230,234,235,236,237,238,239,240,241,242,243}
  elementwise       concat / split: C = 64                             ew-{185,186,187,188,189,190,194,195,196,200,201,202,216,217,218,219,220,221,225,226,227,231,232,233}
  elementwise       cast: n = 1                                        ew-{244,248,253,257}
  elementwise       cast: n = 3                                        ew-{245,249,254,258}
  elementwise       cast: n = 255                                      ew-{246,250,255,259}
  elementwise       cast: n = 257                                      ew-{247,251,256,260}
  elementwise       memcpy: the copy kernel                            ew-{270,271,276}
  elementwise       memcpy: a size that is no multiple of 16           ew-{272,273}
  elementwise       memcpy: misaligned pointers                        ew-{274,275}

Not reachable through the wrappers, on purpose:
  * functional.pyramid_tokens_to_maps passes align_corners=True to both pyramid entry points (the model's only use), so the pyramid sweep
    draws no align_corners=False case; the per-scale resize kernels see both conventions in the resize sweep.
  * the 64-bit index branch of unravel3 / unravel4 (csrc/common.hpp) needs more than 2^32 elements and stays unexercised.
  * msda: the refusals (rows too long for a scatter slab, L = 2, dref with M != 8) are pinned by tests/test_msda_plan_cpu.py and stay out
    of the sweep; FINALIZE and the band kinds do not exist for the (1, 4) build (see MSDA_REGIMES).
  * gconv: emrt_gconv2d has no dilation and no kernel size but 3; maps of 2^31 pixels and more are refused (check_common).  The refusals
    are one separate test without a launch (tests/test_gpu_gconv_fuzz.py).
  * conv: the BatchNorm operand transform (emrt_conv2d_bna) has its own tests and stays out of the sweep (bna_plan is mirrored only to hold
    conv_plan to the recorded table); the dropout epilogue (emrt_conv2d_drop) is the op conv_drop; mode 1 of emrt_conv2d is not what the model runs.  The
    parity-class kernel has no ragged M tile (M / 4 is a multiple of 64 by its own condition) and, like the cross-block split and the pair
    kernel, no scalar epilogue (the host sends those problems elsewhere); the thin kernel takes neither stat_x nor an addend (thin_bwd_ok).
    The weight-gradient kernels' own plan space belongs to tests/test_gpu_wgrad_group.py and the WG8 cases of tests/test_gpu_conv_fuzz.py.
  * loss: a label outside [0, C) that is not the ignore index is outside the contract (include/emrt_hip_loss.h) and loss_in_domain refuses
    it; the Dice entry points stop at 64 classes, so C = 150 runs in the other three families; the 64-bit branch of pixel_of needs 2^32 pixels.
  * step: the learning-rate schedules (tests/test_gpu_adamw.py::test_schedules_on_the_device) and emrt_pack_weights stay out.
  * dropout / conv_drop: emrt_conv2d_drop refuses an output it cannot store in whole 16-byte chunks (conv_drop_vec_ok), so no case has one; no
    statistic is taken on the device -- the model's are checked on the CPU (tests/test_dropout_reference_cpu.py), the device is held to the model.
  * elementwise: the 64-bit index branches (n4 | period4 > 2^32 in the add kernels, unravel3 in add3d / acc3d / concat) need more than 2^32
    elements and stay unexercised; emrt_colsum_acc and emrt_colsum_levels_multi are reductions of csrc/norm.hip and not part of this sweep.
"""
import random

MAX_ELEMS = 400000


def _ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm (training): emrt_bn_stats / emrt_bn_apply / emrt_bn_bwd_reduce / emrt_bn_bwd_dx
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_rowgeom(C):
    """(threads, rows_per_pass) or None.  Mirrors bn_rowgeom (csrc/norm.hip), without the grid size."""
    quads = C // 4
    if quads <= 256:
        if quads == 0 or 256 % quads:
            return None
        return 256, 256 // quads
    if quads <= 512:
        return quads, 1
    return None


def bn_in_domain(case):
    _, N, H, W, C, relu, with_res, _ = case
    return C % 4 == 0 and bn_rowgeom(C) is not None and N * H * W >= 2 and (relu or not with_res)


BN_NARROW = (4, 8, 16, 32, 128, 1024)
BN_WIDE = (1028, 1536, 2044, 2048)


def bn_cases(seed=1101, n=18):
    """(id, N, H, W, C, relu, with_res, seed)"""
    rng = random.Random(seed)
    kinds = ["short", "ragged", "whole-waves", "part-wave", "C=1024", "any"]
    out = []
    while len(out) < n:
        kind = kinds[len(out) % len(kinds)]
        if kind in ("short", "ragged"):
            C = rng.choice((4, 8, 16, 32, 128))
        elif kind == "whole-waves":
            C = rng.choice((1536, 2048))
        elif kind == "part-wave":
            C = rng.choice((1028, 2044))
        elif kind == "C=1024":
            C = 1024
        else:
            C = rng.choice(BN_NARROW + BN_WIDE)
        N, H, W = rng.randint(1, 3), rng.randint(1, 16), rng.randint(1, 16)
        M = N * H * W
        if M < 8 or M > min(600, MAX_ELEMS // C):
            continue
        _, rpp = bn_rowgeom(C)
        if kind == "short" and not (rpp > 1 and M < rpp):
            continue
        if kind == "ragged" and not (rpp > 1 and M > rpp and M % rpp):
            continue
        relu, with_res = rng.choice(((True, True), (True, False), (False, False)))      # as test_batch_norm_train
        out.append(("bn%d-%d" % (seed, len(out)), N, H, W, C, relu, with_res, seed + len(out)))
    return out


def _bn_geo(c):
    """(threads, rows_per_pass, M) of a BatchNorm case"""
    return bn_rowgeom(c[4]) + (c[1] * c[2] * c[3],)


BN_REGIMES = [
    ("256 threads, rows_per_pass > 1, M < rows_per_pass", lambda c: _bn_geo(c)[0] == 256 and 1 < _bn_geo(c)[1] and _bn_geo(c)[2] < _bn_geo(c)[1]),
    ("256 threads, rows_per_pass > 1, M ragged against it", lambda c: _bn_geo(c)[0] == 256 and 1 < _bn_geo(c)[1] < _bn_geo(c)[2] and _bn_geo(c)[2] % _bn_geo(c)[1] != 0),
    ("threads = C/4, whole waves", lambda c: c[4] > 1024 and _bn_geo(c)[0] == c[4] // 4 and _bn_geo(c)[0] % 64 == 0),
    ("threads = C/4, a partial last wave", lambda c: c[4] > 1024 and _bn_geo(c)[0] == c[4] // 4 and _bn_geo(c)[0] % 64 != 0),
    ("C = 1024 (256 threads, one row per pass)", lambda c: c[4] == 1024),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm: emrt_groupnorm_fwd / emrt_groupnorm_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def gn_use_fused(HW, C, G):
    """Mirrors gn_use_fused (csrc/norm.hip): one block per (image, group), else the two-pass statistics + apply kernels."""
    cpg = C // G
    return HW <= 4096 and cpg % 4 == 0 and cpg // 4 <= 64 and 256 % (cpg // 4) == 0 and (cpg // 4) * 64 >= 64


def gn_in_domain(case):
    """the EMRT_REQUIRE of emrt_groupnorm_fwd / _bwd"""
    _, N, H, W, C, G, _, _, _ = case
    return (C % 4 == 0 and C // 4 <= 256 and 256 % (C // 4) == 0 and 0 < G <= 256 and C % G == 0 and (C // G) % 4 == 0
            and N >= 1 and H * W >= 1 and (C // G) * H * W >= 16)


def gn_cases(seed=1202, n=16):
    """(id, N, H, W, C, G, gelu, with_res, seed)"""
    rng = random.Random(seed)
    kinds = ["fused", "hw>4096", "wide-group", "hw=1", "fused", "any"]
    out = []
    while len(out) < n:
        kind = kinds[len(out) % len(kinds)]
        C = 2 ** rng.randint(4, 10)
        N = rng.randint(1, 3)
        H, W = rng.randint(1, 40), rng.randint(1, 40)
        if kind == "hw>4096":
            C, N = rng.choice((16, 32, 64)), 1
            H, W = rng.randint(58, 80), rng.randint(58, 80)
            if not 4096 < H * W <= 5200:
                continue
        elif kind == "wide-group":
            C = rng.choice((512, 1024))
        elif kind == "hw=1":
            H = W = 1
        cpgs = [cpg for cpg in (2 ** e for e in range(2, 11)) if cpg <= C and C // cpg <= 256]
        if kind == "wide-group":
            cpgs = [cpg for cpg in cpgs if cpg > 256]
        elif kind == "fused":
            cpgs = [cpg for cpg in cpgs if cpg <= 256]
        G = C // rng.choice(cpgs)
        if N * H * W * C > MAX_ELEMS or (C // G) * H * W < 16:
            continue
        gelu, with_res = rng.random() < 0.5, rng.random() < 0.5
        out.append(("gn%d-%d" % (seed, len(out)), N, H, W, C, G, gelu, with_res, seed + len(out)))
    return out


GN_REGIMES = [
    ("fused (one block per image and group)", lambda c: gn_use_fused(c[2] * c[3], c[4], c[5])),
    ("two-pass because HW > 4096", lambda c: not gn_use_fused(c[2] * c[3], c[4], c[5]) and c[2] * c[3] > 4096),
    ("two-pass because C/G > 256", lambda c: not gn_use_fused(c[2] * c[3], c[4], c[5]) and c[4] // c[5] > 256),
    ("HW = 1", lambda c: c[2] * c[3] == 1),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm over token levels: emrt_groupnorm_levels_fwd / _bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def gn_rows_ok(C, G):
    """Mirrors gn_rows_ok (csrc/norm.hip) for dense token tensors (ld = C, bs = Lv * C): the row-major statistics + apply pair, else one
    block per (level, image, group)."""
    return C == 8 * G and 256 % G == 0 and C <= 256


def gnl_in_domain(case):
    _, B, hws, C, G, _, _, _ = case
    return G > 0 and C % G == 0 and gn_use_fused(1, C, G) and 1 <= len(hws) <= 4 and all(1 <= n <= 4096 for n in hws) and B >= 1


GNL_PAIRS = ((256, 32), (64, 4))          # the model's, and one other pair gn_use_fused(1, C, G) accepts (16 channels per group)


def gnl_cases(seed=1303, n=8):
    """(id, B, level sizes, C, G, gelu, with_res, seed)"""
    rng = random.Random(seed)
    kinds = ["L=1", "L=4", "one-row", "any"]
    out = []
    while len(out) < n:
        kind = kinds[len(out) % len(kinds)]
        C, G = GNL_PAIRS[(len(out) // 2) % 2]
        L = {"L=1": 1, "L=4": 4}.get(kind, rng.randint(1, 4))
        hws = [rng.choice((1, rng.randint(2, 30), rng.randint(31, 400), rng.randint(401, 4096))) for _ in range(L)]      # not sorted
        if kind == "one-row":
            hws[rng.randrange(L)] = 1
        B = rng.randint(1, 2)
        if B * sum(hws) * C > MAX_ELEMS or (C // G) * min(hws) < 16:
            continue
        out.append(("gnl%d-%d" % (seed, len(out)), B, tuple(hws), C, G, rng.random() < 0.5, rng.random() < 0.5, seed + len(out)))
    return out


GNL_REGIMES = [
    ("L = 1", lambda c: len(c[2]) == 1),
    ("L = 4", lambda c: len(c[2]) == 4),
    ("a level of one row", lambda c: 1 in c[2]),
    ("row-major kernels (C = 8 G)", lambda c: gn_rows_ok(c[3], c[4])),
    ("block per (level, image, group)", lambda c: not gn_rows_ok(c[3], c[4])),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm: emrt_layernorm_fwd / emrt_layernorm_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_bwd_blocks(rows, C, rows_knob=0, max_blocks_knob=0, threads_knob=512):
    """(blocks, capped).  Mirrors ln_bwd_blocks (csrc/norm.hip) with the tuning knobs ln_bwd_rows / ln_bwd_max_blocks / ln_bwd_threads;
    capped: the block cap, not the row count, decides the grid, so every block loops over more rows than `per`."""
    wide = C <= 256 and threads_knob >= 512
    per = rows_knob if rows_knob > 0 else (64 if wide else 32)
    cap = max_blocks_knob if max_blocks_knob > 0 else (256 if wide else 512)
    blocks = _ceil_div(rows, per)
    capped = blocks > cap
    return max(1, min(blocks, cap)), capped


def ln_in_domain(case):
    _, B, L, C, form, max_blocks, rows_knob, _ = case
    return C % 4 == 0 and 12 <= C <= 1024 and B * L >= 1 and form in LN_FORMS and max_blocks >= 0 and rows_knob >= 0


LN_CS = (12, 64, 100, 252, 256, 260, 512, 1000, 1024)
LN_FORMS = ("a", "a+b", "a+b,post")


def ln_cases(seed=1404, n=18):
    """(id, B, L, C, form, ln_bwd_max_blocks, ln_bwd_rows, seed); the knobs are 0 (library default) except in the block-cap cases"""
    rng = random.Random(seed)
    kinds = ["C<256", "C=256", "C>256 ragged", "C=1024", "rows%4", "rows=1", "cap", "any", "any"]
    out = []
    while len(out) < n:
        kind = kinds[len(out) % len(kinds)]
        C = {"C<256": rng.choice((12, 64, 100, 252)), "C=256": 256, "C>256 ragged": rng.choice((260, 1000)), "C=1024": 1024}.get(kind, rng.choice(LN_CS))
        B, L = rng.randint(1, 3), rng.randint(1, 233)
        if kind == "rows=1":
            B = L = 1
        rows = B * L
        if rows * C > MAX_ELEMS or (kind == "rows%4" and rows % 4 == 0):
            continue
        knobs = (0, 0)
        if kind == "cap":
            knobs = rng.choice(((2, 0), (3, 8)))
            if not ln_bwd_blocks(rows, C, knobs[1], knobs[0])[1]:
                continue
        out.append(("ln%d-%d" % (seed, len(out)), B, L, C, LN_FORMS[len(out) % 3], knobs[0], knobs[1], seed + len(out)))
    return out


LN_REGIMES = [
    ("C < 256 (a partial pass)", lambda c: c[3] < 256),
    ("C = 256 (one whole pass)", lambda c: c[3] == 256),
    ("C > 256 with a ragged last pass", lambda c: c[3] > 256 and c[3] % 256 != 0),
    ("C = 1024", lambda c: c[3] == 1024),
    ("rows % 4 != 0", lambda c: (c[1] * c[2]) % 4 != 0),
    ("rows = 1", lambda c: c[1] * c[2] == 1),
    ("backward blocks loop under the block cap", lambda c: ln_bwd_blocks(c[1] * c[2], c[3], c[6], c[5])[1]),
] + [("form ln(%s)" % f, (lambda f_: lambda c: c[4] == f_)(f)) for f in LN_FORMS]


# ---------------------------------------------------------------------------------------------------------------------------------
# bilinear resize: emrt_resize_bilinear_fwd / _bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def vec_width(C, fp32, widths=(8, 4, 1)):
    """Channels per access for a dense, aligned map.  Mirrors the v8 / v4 / scalar choice of emrt_resize_bilinear_fwd / _bwd (8 only for the
    16-bit types), emrt_maxpool_fwd (widths = (8, 1), every type) and emrt_maxpool_bwd / emrt_adaptive_avgpool_bwd (widths = (4, 1))."""
    for v in widths:
        if C % v == 0 and not (v == 8 and fp32 and 4 in widths):
            return v
    return 1


def resize_bwd_wide(C, IH, IW, OH, OW):
    """Mirrors the block-per-source-pixel condition of emrt_resize_bilinear_bwd (RBW_THREADS = 1024)."""
    return C % 4 == 0 and C // 4 <= 1024 and OH * OW >= 16 * IH * IW


def resize_in_domain(case):
    _, N, IH, IW, C, OH, OW, _, add, nchw, _ = case
    return min(N, IH, IW, C, OH, OW) >= 1 and not (add and nchw)


RESIZE_CS = (3, 6, 7, 8, 20, 64)


def resize_cases(seed=1505, n=26):
    """(id, N, IH, IW, C, OH, OW, align_corners, add_t, out_nchw_f32, seed)"""
    rng = random.Random(seed)
    kinds = ["up", "down", "mixed", "identity", "in 1x1", "out 1x1", "nchw", "wide", "C%8", "C%4", "scalar", "any", "any"]
    out = []
    while len(out) < n:
        kind = kinds[len(out) % len(kinds)]
        IH, IW, OH, OW = (rng.randint(1, 40) for _ in range(4))
        C = {"C%8": rng.choice((8, 64)), "C%4": 20, "scalar": rng.choice((3, 6, 7)), "wide": rng.choice((8, 20, 64))}.get(kind, rng.choice(RESIZE_CS))
        if kind == "identity":
            OH, OW = IH, IW
        elif kind == "in 1x1":
            IH = IW = 1
        elif kind == "out 1x1":
            OH = OW = 1
        elif kind == "wide":
            IH, IW = rng.randint(1, 9), rng.randint(1, 9)
            OH, OW = rng.randint(4 * IH, 40), rng.randint(4 * IW, 40)
        elif kind == "up" and not (OH >= IH and OW >= IW and (OH, OW) != (IH, IW)):
            continue
        elif kind == "down" and not (OH <= IH and OW <= IW and (OH, OW) != (IH, IW)):
            continue
        elif kind == "mixed" and not ((OH > IH and OW < IW) or (OH < IH and OW > IW)):
            continue
        nchw = kind == "nchw" or (kind == "any" and rng.random() < 0.3)
        add = (not nchw) and rng.random() < 0.5
        out.append(("rs%d-%d" % (seed, len(out)), rng.randint(1, 3), IH, IW, C, OH, OW, rng.random() < 0.5, add, nchw, seed + len(out)))
    return out


RESIZE_REGIMES = [
    ("up on both axes", lambda c: c[5] >= c[2] and c[6] >= c[3] and (c[5], c[6]) != (c[2], c[3])),
    ("down on both axes", lambda c: c[5] <= c[2] and c[6] <= c[3] and (c[5], c[6]) != (c[2], c[3])),
    ("mixed: up on one axis, down on the other", lambda c: (c[5] > c[2] and c[6] < c[3]) or (c[5] < c[2] and c[6] > c[3])),
    ("identity", lambda c: (c[5], c[6]) == (c[2], c[3])),
    ("down with align_corners=False", lambda c: not c[7] and (c[5] < c[2] or c[6] < c[3])),
    ("1-pixel input", lambda c: c[2] == c[3] == 1),
    ("1-pixel output", lambda c: c[5] == c[6] == 1),
    ("NHWC, 8 channels per access (bf16)", lambda c: not c[9] and vec_width(c[4], False) == 8),
    ("NHWC, 4 channels per access", lambda c: not c[9] and vec_width(c[4], True) == 4 and vec_width(c[4], False) == 4),
    ("NHWC, scalar", lambda c: not c[9] and vec_width(c[4], True) == 1),
    ("backward: block per source pixel", lambda c: not c[9] and resize_bwd_wide(c[4], c[2], c[3], c[5], c[6])),
    ("fp32 NCHW output and its two-kernel backward", lambda c: c[9]),
    ("fused addend", lambda c: c[8]),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# max pooling: emrt_maxpool_fwd / emrt_maxpool_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def pool_out(S, k, stride, pad):
    return (S + 2 * pad - k) // stride + 1


def maxpool_in_domain(case):
    _, N, H, W, C, k, stride, pad, _ = case
    return (0 < k <= 15 and stride > 0 and 0 <= pad < k and pad <= k // 2          # (pad <= k // 2: torch's limit, which the reference needs)
            and pool_out(H, k, stride, pad) >= 1 and pool_out(W, k, stride, pad) >= 1 and H + 2 * pad >= k and W + 2 * pad >= k)


MAXPOOL_CS = (3, 4, 12, 8, 64)


def maxpool_cases(seed=1606, n=18):
    """(id, N, H, W, C, k, stride, pad, seed)"""
    rng = random.Random(seed)
    kinds = ["stride<k", "stride=k", "stride>k", "k=1", "any", "any"]
    out = []
    while len(out) < n:
        kind = kinds[len(out) % len(kinds)]
        k = 7 if len(out) == n - 1 else (1 if kind == "k=1" else rng.randint(1, 5))          # one k = 7
        stride = rng.randint(1, k + 1)
        pad = rng.randint(0, k // 2)
        H, W = rng.randint(3, 30), rng.randint(3, 30)
        if (kind == "stride<k" and not stride < k) or (kind == "stride=k" and stride != k) or (kind == "stride>k" and not stride > k):
            continue
        if H + 2 * pad < k or W + 2 * pad < k:
            continue
        out.append(("mp%d-%d" % (seed, len(out)), rng.randint(1, 3), H, W, MAXPOOL_CS[len(out) % len(MAXPOOL_CS)], k, stride, pad, seed + len(out)))
    return out


MAXPOOL_REGIMES = [
    ("stride < k (windows overlap)", lambda c: c[6] < c[5]),
    ("stride = k", lambda c: c[6] == c[5]),
    ("stride > k (pixels in no window)", lambda c: c[6] > c[5]),
    ("k = 1", lambda c: c[5] == 1),
    ("k = 7", lambda c: c[5] == 7),
    ("forward 8 channels per thread, backward 4", lambda c: vec_width(c[4], True, (8, 1)) == 8),
    ("forward scalar, backward 4 channels per thread", lambda c: vec_width(c[4], True, (8, 1)) == 1 and vec_width(c[4], True, (4, 1)) == 4),
    ("scalar both ways", lambda c: vec_width(c[4], True, (4, 1)) == 1),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# adaptive average pooling to tokens: emrt_adaptive_avgpool_fwd / _bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def pool_split(H, W, C, Ctot, scales):
    """Mirrors the split-bin choice of emrt_adaptive_avgpool_fwd (pool_split_plan and the vector condition in front of it, csrc/spatial.hip)
    for a channel slice [.., :C] of a dense [N, H, W, Ctot] map: several blocks per bin."""
    kmin = min(scales)
    big = ((H + kmin - 1) // kmin + 1) * ((W + kmin - 1) // kmin + 1)
    cq = C // 4
    return Ctot % 4 == 0 and C % 4 == 0 and cq <= 256 and (cq & (cq - 1)) == 0 and big >= 512


def pool_bwd_kernel(H, W, C, scales):
    """'table' | 'gather' | 'scalar'.  Mirrors the kernel choice of emrt_adaptive_avgpool_bwd (dense gradients)."""
    if C % 4:
        return "scalar"
    return "table" if H + W <= 512 and all(k <= min(H, W) for k in scales) else "gather"


def adaptive_in_domain(case):
    _, N, H, W, C, Ctot, scales, _ = case
    return min(N, H, W, C) >= 1 and Ctot >= C and 1 <= len(scales) <= 4 and len(set(scales)) == len(scales) and all(1 <= k <= 8 for k in scales)


ADAPTIVE_CS = (4, 8, 64, 100, 6)          # functional.adaptive_avgpool_tokens lets C % 4 != 0 through: C = 6 takes the scalar kernels


def adaptive_cases(seed=1707, n=14):
    """(id, N, H, W, C, Ctot, scales, seed): the input is the channel slice [.., :C] of a [N, H, W, Ctot] buffer"""
    rng = random.Random(seed)
    kinds = ["H or W < k", "non-square", "split", "scalar", "any"]
    out = []
    while len(out) < n:
        kind = kinds[len(out) % len(kinds)]
        scales = tuple(rng.sample(range(1, 9), rng.randint(1, 4)))
        H, W = rng.randint(1, 50), rng.randint(1, 50)
        C = {"split": rng.choice((4, 8, 64)), "scalar": 6}.get(kind, rng.choice(ADAPTIVE_CS))
        if kind == "H or W < k":
            if rng.random() < 0.5:
                H = rng.randint(1, max(1, max(scales) - 1))
            else:
                W = rng.randint(1, max(1, max(scales) - 1))
        Ctot = C + (rng.choice((0, 4, 8, 60)) if C % 4 == 0 else rng.choice((0, 2, 5)))
        N = rng.randint(1, 3)
        if N * H * W * Ctot > MAX_ELEMS:
            continue
        if (kind == "H or W < k" and not min(H, W) < max(scales)) or (kind == "non-square" and H == W) or (kind == "split" and not pool_split(H, W, C, Ctot, scales)):
            continue
        out.append(("ap%d-%d" % (seed, len(out)), N, H, W, C, Ctot, scales, seed + len(out)))
    return out


ADAPTIVE_REGIMES = [
    ("H or W < k", lambda c: min(c[2], c[3]) < max(c[6])),
    ("non-square map", lambda c: c[2] != c[3]),
    ("forward: several blocks per bin", lambda c: pool_split(c[2], c[3], c[4], c[5], c[6])),
    ("forward: one block per bin", lambda c: not pool_split(c[2], c[3], c[4], c[5], c[6])),
    ("scalar path (C % 4 != 0)", lambda c: c[4] % 4 != 0),
    ("backward: two-bin table", lambda c: pool_bwd_kernel(c[2], c[3], c[4], c[6]) == "table"),
    ("backward: general gather", lambda c: pool_bwd_kernel(c[2], c[3], c[4], c[6]) == "gather"),
    ("input is a slice of a wider buffer", lambda c: c[5] > c[4]),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# pyramid token maps: emrt_pyramid_resize_fwd / _bwd (functional.pyramid_tokens_to_maps)
# ---------------------------------------------------------------------------------------------------------------------------------
def pyramid_in_domain(case):
    _, B, C, scales, OH, OW, grouped, _ = case
    return (B >= 1 and C % 4 == 0 and 4 <= C <= 256 and 1 <= len(scales) <= 4 and len(set(scales)) == len(scales)
            and all(1 <= k <= 8 for k in scales) and OH >= 4 * max(scales) and OW >= 4 * max(scales))


def pyramid_grouped(C, scales, OH, OW, esz, knob):
    """Mirrors the `grouped` choice of functional.pyramid_tokens_to_maps and of its backward, for maps that are the channel slices
    C .. C * (len(scales) + 1) of one 16-byte aligned NHWC concat buffer (and gradients that are the same slices of another): the knob
    (Context.pyramid_group), at most four scales, C % 4 == 0, and every slice on a 16-byte boundary, which is C * esz % 16 == 0; the
    row and image strides are multiples of C.  The backward also wants OH * OW >= 16 k^2, which the entry point's OH, OW >= 4 max(k)
    implies.  esz = bytes per element: at C = 4 or 12 the bf16 slices start on an 8-byte boundary and each scale gets its own launch."""
    return (knob and len(scales) <= 4 and C % 4 == 0 and (C * esz) % 16 == 0
            and all(OH * OW >= 16 * k * k for k in scales))


def pyramid_cases(seed=1808, n=12):
    """(id, B, C, scales, OH, OW, knob, seed); knob = Context.pyramid_group: one launch per direction where pyramid_grouped allows
    it, or always one per scale"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        scales = tuple(rng.sample(range(1, 9), rng.randint(1, 4)))
        kmax = max(scales)
        OH, OW = rng.randint(4 * kmax, 4 * kmax + 12), rng.randint(4 * kmax, 4 * kmax + 12)
        B, C = rng.randint(1, 3), rng.choice((4, 8, 12, 16, 32, 64, 128, 256))
        if B * OH * OW * C * (len(scales) + 1) > MAX_ELEMS:
            continue
        out.append(("py%d-%d" % (seed, len(out)), B, C, scales, OH, OW, len(out) % 2 == 0, seed + len(out)))
    return out


PYRAMID_REGIMES = [
    ("one launch per direction, fp32 and bf16", lambda c: pyramid_grouped(c[2], c[3], c[4], c[5], 4, c[6]) and pyramid_grouped(c[2], c[3], c[4], c[5], 2, c[6])),
    ("one launch in fp32, per scale in bf16 (8-byte slices)", lambda c: pyramid_grouped(c[2], c[3], c[4], c[5], 4, c[6]) and not pyramid_grouped(c[2], c[3], c[4], c[5], 2, c[6])),
    ("per-scale fallback by the knob", lambda c: not c[6]),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# sliding-window glue: emrt_window_accumulate
# ---------------------------------------------------------------------------------------------------------------------------------
def window_vec4(W, cw, origins_yx):
    """Mirrors the vec4 condition of emrt_window_accumulate (csrc/spatial.hip) for 16-byte aligned buffers: four x per thread."""
    return W % 4 == 0 and cw % 4 == 0 and all(x % 4 == 0 for _, x in origins_yx)


# One image: classes, H, W, window height and width; irregular overlaps (pixels covered 1, 2, 3 and 4 times) and the columns from x = 20 on
# covered by no window.  "grid": every origin's x, cw and W are multiples of 4; "odd": the same windows with one origin of each of the two
# calls moved by one pixel, so that both calls leave the vec4 kernel.
WINDOW_IMAGE = dict(C=5, H=20, W=24, ch=8, cw=8)
WINDOW_ORIGINS = {
    "grid": ((0, 0), (0, 4), (4, 0), (4, 4), (2, 8), (11, 0), (12, 12), (9, 8)),
    "odd": ((0, 0), (0, 4), (4, 1), (4, 4), (2, 8), (11, 1), (12, 12), (9, 8)),
}
WINDOW_SPLIT = 5          # the windows go in two calls ([:5], [5:]) into the same final / count, as slide_inference's max_batch chunks do


def window_cover(origins_yx, H, W, ch, cw):
    """times each pixel is covered: [H][W] list of ints"""
    cov = [[0] * W for _ in range(H)]
    for y0, x0 in origins_yx:
        for y in range(y0, y0 + ch):
            for x in range(x0, x0 + cw):
                cov[y][x] += 1
    return cov


# ---------------------------------------------------------------------------------------------------------------------------------
# attention: emrt_mha_fwd / emrt_mha_bwd (tests/test_gpu_mha_fuzz.py; the float64 reference and the bounds are tests/mha_reference.py)
# ---------------------------------------------------------------------------------------------------------------------------------
MHA_MAXL = 128


def mha_path(is16bit, L, valu_knob, aligned):
    """0: VALU kernels (`probs` = L x L probabilities), 1: MFMA kernels (`probs` = row statistics).  Mirrors `mfma` of emrt_mha_fwd
    (csrc/attn.hip) for row strides that are multiples of 8; aligned: q, k, v on 16-byte and o on 8-byte boundaries."""
    return int(bool(is16bit and not valu_knob and L >= 2 and aligned))


def mha_bwd_stages_probs(L):
    """Mirrors use_sp of emrt_mha_bwd: the VALU backward keeps the dropped probabilities in LDS (else it re-derives them from `probs`)."""
    return (4 * L * 36 + 2 * L * (L + 1)) * 4 <= 159 * 1024


def mha_tiles(L):
    """16-row tiles of the MFMA kernels (nt); they walk k in pairs of tiles, so an odd count leaves the last k-step half padding"""
    return (L + 15) // 16


def mha_fwd_chunks(L):
    """32-row chunks of the VALU forward (nchunk): blocks per (batch, head)"""
    return (L + 31) // 32


def mha_in_domain(case):
    _, B, M, L, regime, p, layout, _ = case
    return (B >= 1 and M >= 1 and 1 <= L <= MHA_MAXL and regime in MHA_INPUTS and layout in MHA_LAYOUTS and 0.0 <= p < 1.0
            and (p == 0.0 or regime == "ordinary"))


MHA_LS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 109, 110, 111, 112, 113, 127, 128)
MHA_DROP_LS = (17, 33, 49, 110, 111, 113, 127, 128)
MHA_MS = (1, 2, 3, 4, 8)
MHA_INPUTS = ("ordinary", "peaked", "negative", "lastkey")          # tests/mha_reference.make_inputs
# fused: through functional.mha (q | k in one buffer with ld = 2 E, the rest ld = E); split: the C entry points with q, k, v in three buffers
# of row strides E, E + 8, 2 E + 16; offset8: the same with q 8 bytes off a 16-byte boundary in bf16 (path 0 by the alignment rule; an fp32
# call has no such rule and runs the case as `split`).  Both direct layouts write o, dq, dk, dv into wider pre-filled buffers.
MHA_LAYOUTS = ("fused", "split", "offset8")


def mha_cases(seed=1909):
    """(id, B, M, L, input regime, pdrop, layout, seed): every length of MHA_LS twice without dropout (another input regime and another
    layout the second time), then MHA_DROP_LS x p in {0.1, 0.5} with ordinary inputs"""
    rng = random.Random(seed)
    out = []

    def add(L, regime, p, layout):
        while True:
            B, M = rng.randint(1, 4), rng.choice(MHA_MS)
            if B * M * L * L <= MAX_ELEMS:
                break
        out.append(("mha%d-%d" % (seed, len(out)), B, M, L, regime, p, layout, seed + len(out)))

    n = len(MHA_LS)
    for i in range(2 * n):
        add(MHA_LS[i % n], MHA_INPUTS[i % 4], 0.0, MHA_LAYOUTS[(i + i // n) % 3])
    for i, L in enumerate(MHA_DROP_LS):
        for j, p in enumerate((0.1, 0.5)):
            add(L, "ordinary", p, MHA_LAYOUTS[(i + j) % 3])
    return out


MHA_REGIMES = [
    ("L = 1 (VALU kernels in every dtype)", lambda c: c[3] == 1),
    ("odd tile count (last k-step half padding)", lambda c: c[3] >= 2 and mha_tiles(c[3]) % 2 == 1),
    ("L % 16 = 0", lambda c: c[3] % 16 == 0),
    ("L % 16 = 1", lambda c: c[3] % 16 == 1 and c[3] > 1),
    ("L % 16 = 15", lambda c: c[3] % 16 == 15),
    ("L % 4 != 0 (ragged lane quads)", lambda c: c[3] % 4 != 0),
    ("ragged last forward chunk", lambda c: c[3] % 32 != 0 and mha_fwd_chunks(c[3]) > 1),
    ("VALU backward stages Pd in LDS", lambda c: mha_bwd_stages_probs(c[3])),
    ("VALU backward re-derives Pd", lambda c: not mha_bwd_stages_probs(c[3])),
    ("M = 1", lambda c: c[2] == 1),
    ("M not in (1, 8)", lambda c: c[2] not in (1, 8)),
    ("B = 1", lambda c: c[1] == 1),
] + [("inputs: %s" % r, (lambda r_: lambda c: c[4] == r_ and c[5] == 0.0)(r)) for r in MHA_INPUTS] + [
    ("dropout, Pd staged in LDS", lambda c: c[5] > 0 and mha_bwd_stages_probs(c[3])),
    ("dropout, Pd re-derived", lambda c: c[5] > 0 and not mha_bwd_stages_probs(c[3])),
    ("dropout, odd tile count", lambda c: c[5] > 0 and mha_tiles(c[3]) % 2 == 1),
] + [("layout: %s" % l, (lambda l_: lambda c: c[6] == l_)(l)) for l in MHA_LAYOUTS] + [
    ("dropout, layout: %s" % l, (lambda l_: lambda c: c[5] > 0 and c[6] == l_)(l)) for l in MHA_LAYOUTS]


# ---------------------------------------------------------------------------------------------------------------------------------
# deformable attention: emrt_msda_fwd / emrt_msda_bwd (tests/test_gpu_msda_fuzz.py; the float64 reference and the bounds are
# tests/msda_reference.py).  Unlike the lists above this one is written out: a case is there to reach named kernels, and `expect` says
# which -- data, confirmed against the planner (emrt_msda_plan, no GPU needed) by tests/test_msda_reference_cpu.py.
# ---------------------------------------------------------------------------------------------------------------------------------
MSDA_MAX_ELEMS = 1500000          # per tensor; apart from MAX_ELEMS: the smallest pyramid the row-band kernels take has Lv ~ 2500
MSDA_BUILDS = ((3, 6), (4, 4), (3, 4), (1, 4))          # (levels, points) of with_levels_points (csrc/msda.hip)
MSDA_KINDS = ("FWD_GLOBAL", "FWD_LDS", "FWD_BAND", "GRAD_GLOBAL", "GRAD_LDS", "GRAD_BAND", "ABSMAX", "SCATTER_MF", "SCATTER_LDS", "FINALIZE")
MSDA_INPUTS = ("ordinary", "far", "border", "bandedge", "centres", "spike", "lastquery")          # tests/msda_reference.make_inputs
# dense: through functional.msda.  strided: the C entry points; value is a channel slice of a wider buffer (ldv = 32 M + 64, v_bs padded by
# a further 8 ldv), ldo = 3 M L P + 2, every output in a pre-filled buffer
MSDA_LAYOUTS = ("dense", "strided")
# reference points shared by the batch or one set per batch element, one point per query or one per level; "+dref": their gradient is asked for
MSDA_REFMODES = ("shared-1", "batch-1", "shared-L", "batch-L")
MSDA_LDS_MAX = 159 * 1024
MSDA_KNOBS = ("msda_fwd_global", "msda_bwd_global", "msda_bwd_dref_lds", "msda_scatter_mfma", "msda_scatter_qsplit", "msda_scatter_cuts",
              "msda_band_halo", "msda_mf_bands", "msda_lds_min_pairs")


def msda_band_geometry(shapes, B, M, halo_knob=0):
    """(NB, halo, slab bytes) of the row-band plan of a self-attention call over `shapes`, (0, 0, 0) when the whole (batch, head) slab fits
    in LDS or no band plan exists.  Mirrors msda_band_plan and the slab test of msda_plan (csrc/msda.hip)."""
    L = len(shapes)
    guard = max(w for _, w in shapes) + 2
    if L < 2 or (sum(h * w for h, w in shapes) + 2 * guard) * 64 <= MSDA_LDS_MAX:
        return 0, 0, 0
    NB = 2
    while NB <= 64:
        if any(h % NB for h, _ in shapes):
            break
        if NB * B * M < 192 and NB * 2 <= 64 and not any(h % (NB * 2) for h, _ in shapes):
            NB *= 2
            continue
        for halo in range(halo_knob if halo_knob > 0 else 7, 2, -1):
            npx = guard
            for h, w in shapes:
                npx = ((npx + 15) & ~15) + min(h // NB + 2 * halo, h) * w
            slab = ((npx + guard + 15) >> 4 << 4) * 64
            if slab <= MSDA_LDS_MAX:
                return NB, halo, slab
        NB *= 2
    return 0, 0, 0


def msda_scatter_max_npix(shapes):
    """most pixels of one range of the integer scatter's LDS slab.  Mirrors msda_max_npix (csrc/msda.hip)."""
    return ((160 * 1024 - 20480) // (33 * 4) - 2 * (max(w for _, w in shapes) + 2)) & ~3


def msda_lq(case):
    return case[4] or sum(h * w for h, w in case[3])


def msda_in_domain(case):
    _, B, M, shapes, Lq, P, regime, layout, refmode, knobs, expect, _ = case
    dtype, fwd, bwd = expect
    base, _, dref = refmode.partition("+")
    Lv = sum(h * w for h, w in shapes)
    pow2 = all(h & (h - 1) == 0 and w & (w - 1) == 0 for h, w in shapes)
    return ((len(shapes), P) in MSDA_BUILDS and B >= 1 and M >= 1 and B * max(Lv, Lq or Lv) * M * 32 <= MSDA_MAX_ELEMS
            and regime in MSDA_INPUTS and layout in MSDA_LAYOUTS and base in MSDA_REFMODES and dref in ("", "dref")
            and (not dref or (M == 8 and dtype != "f16")) and set(knobs) <= set(MSDA_KNOBS)
            and dtype in ("f32", "bf16", "f16") and (bwd is None) == (dtype == "f16") and set(fwd) | set(bwd or ()) <= set(MSDA_KINDS)
            and (regime != "bandedge" or (Lq is None and msda_band_geometry(shapes, B, M, knobs.get("msda_band_halo", 0))[0] > 0))
            and (regime != "centres" or pow2)
            and all(h * w <= msda_scatter_max_npix(shapes) * h for h, w in shapes))          # (a row fits a scatter slab: else a refusal)


MSDA_BAND4 = ((48, 40), (24, 20), (12, 10))          # NB = 4, halo = 7
MSDA_BAND4_4 = MSDA_BAND4 + ((6, 5),)
MSDA_BAND2A = ((44, 45), (22, 23), (10, 11))         # NB = 2, odd widths, segments that are no multiples of 16
MSDA_BAND2A_4 = MSDA_BAND2A + ((4, 5),)
MSDA_BAND2B = ((50, 40), (26, 20), (14, 10))         # NB = 2
MSDA_T3 = ((3, 5), (2, 3), (1, 1))
MSDA_T4 = MSDA_T3 + ((1, 2),)
MSDA_T1 = ((3, 5),)
MSDA_ODD3 = ((13, 17), (7, 9), (4, 5))
MSDA_ODD4 = MSDA_ODD3 + ((2, 3),)
MSDA_P2_3 = ((16, 16), (8, 8), (4, 4))
MSDA_P2_4 = MSDA_P2_3 + ((2, 2),)
MSDA_MID3 = ((20, 18), (10, 9), (5, 5))
MSDA_MF3 = ((7, 10), (4, 5), (2, 3))
MSDA_MF4 = MSDA_MF3 + ((1, 2),)
MSDA_FIN3 = ((32, 28), (16, 14), (8, 7))             # the smallest pyramid whose small levels' scatter blocks are split by queries (FINALIZE)
MSDA_FIN4 = MSDA_FIN3 + ((4, 4),)

# (B, M, shapes, Lq or None (= Lv: self-attention over the pyramid), P, input regime, layout, refmode, knobs, (dtype, forward kinds, backward kinds))
_MSDA_ROWS = (
    (1, 8, MSDA_BAND4, None, 6, "ordinary", "dense", "shared-1", {}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND4, None, 6, "far", "dense", "shared-L", {"msda_band_halo": 3}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND4, None, 6, "bandedge", "strided", "shared-1", {"msda_band_halo": 3}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND2A, None, 6, "lastquery", "dense", "batch-1", {}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND2B, None, 6, "bandedge", "dense", "shared-1", {}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND2A, None, 6, "border", "strided", "batch-L", {}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (2, 4, MSDA_BAND4, None, 6, "ordinary", "strided", "batch-1", {}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND4, None, 6, "ordinary", "dense", "batch-L+dref", {}, ("bf16", ("FWD_BAND",), ("GRAD_GLOBAL", "ABSMAX", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND4_4, None, 4, "ordinary", "dense", "batch-L", {}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND4_4, None, 4, "bandedge", "strided", "shared-L", {"msda_band_halo": 3}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND2A_4, None, 4, "spike", "dense", "shared-1", {}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND4, None, 4, "far", "dense", "shared-1", {}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND2B, None, 4, "bandedge", "strided", "batch-1", {}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND2A, None, 4, "lastquery", "dense", "shared-L", {"msda_band_halo": 3}, ("bf16", ("FWD_BAND",), ("GRAD_BAND", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_BAND4, None, 6, "ordinary", "strided", "shared-1", {}, ("f16", ("FWD_BAND",), None)),
    (1, 8, MSDA_BAND2A_4, None, 4, "border", "dense", "shared-L", {"msda_band_halo": 3}, ("f16", ("FWD_BAND",), None)),
    (1, 8, MSDA_BAND2B, None, 4, "bandedge", "dense", "shared-1", {}, ("f16", ("FWD_BAND",), None)),
    (1, 8, MSDA_T3, 1, 6, "ordinary", "dense", "shared-1", {"msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (3, 3, MSDA_T3, 129, 6, "lastquery", "strided", "batch-1", {"msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (2, 8, MSDA_P2_3, None, 6, "centres", "dense", "batch-L+dref", {}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (2, 8, MSDA_P2_3, 110, 6, "ordinary", "dense", "shared-1+dref", {"msda_bwd_dref_lds": 0, "msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_GLOBAL", "SCATTER_MF"))),
    (2, 8, MSDA_P2_3, 113, 6, "lastquery", "strided", "shared-L+dref", {"msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (2, 16, MSDA_ODD3, None, 6, "ordinary", "dense", "shared-1", {}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (3, 1, MSDA_ODD3, 129, 6, "far", "strided", "shared-L", {"msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (1, 2, MSDA_ODD3, 200, 6, "border", "dense", "batch-1", {"msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (1, 4, MSDA_MID3, 1041, 6, "spike", "dense", "shared-1", {}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (1, 8, MSDA_T4, 1, 4, "far", "strided", "shared-1", {"msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (2, 8, MSDA_P2_4, None, 4, "centres", "strided", "shared-L+dref", {}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (1, 8, MSDA_ODD4, None, 4, "border", "dense", "batch-1+dref", {"msda_bwd_dref_lds": 0, "msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_GLOBAL", "SCATTER_MF"))),
    (3, 2, MSDA_T3, 129, 4, "ordinary", "strided", "batch-L", {"msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (3, 8, ((16, 12), (8, 6), (4, 3)), 145, 4, "far", "dense", "batch-L+dref", {}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (1, 8, MSDA_T1, 1, 4, "border", "dense", "shared-1", {"msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (2, 8, ((16, 16),), None, 4, "centres", "dense", "batch-1+dref", {}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (2, 3, ((13, 17),), 129, 4, "lastquery", "strided", "shared-1", {"msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (2, 8, MSDA_ODD3, None, 6, "ordinary", "strided", "batch-1", {"msda_lds_min_pairs": 0}, ("f16", ("FWD_LDS",), None)),
    (1, 4, ((9, 11),), 77, 4, "border", "dense", "shared-1", {"msda_lds_min_pairs": 0}, ("f16", ("FWD_LDS",), None)),
    (2, 8, MSDA_P2_4, None, 4, "centres", "dense", "shared-L", {}, ("f16", ("FWD_LDS",), None)),
    (2, 8, MSDA_T3, 37, 6, "ordinary", "dense", "batch-L+dref", {}, ("f32", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "SCATTER_LDS"))),
    (1, 8, MSDA_MID3, 1041, 6, "lastquery", "strided", "shared-1+dref", {}, ("f32", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "ABSMAX", "SCATTER_LDS"))),
    (1, 8, MSDA_BAND4, None, 6, "far", "dense", "shared-1", {}, ("f32", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "ABSMAX", "SCATTER_LDS"))),
    (2, 4, ((12, 10), (6, 5), (3, 3)), 1025, 6, "spike", "dense", "batch-1", {"msda_fwd_global": 1, "msda_bwd_global": 1}, ("bf16", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "ABSMAX", "SCATTER_MF"))),
    (1, 16, MSDA_ODD3, 1040, 6, "ordinary", "dense", "shared-L", {"msda_fwd_global": 1, "msda_bwd_global": 1}, ("bf16", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "SCATTER_MF"))),
    (2, 3, MSDA_ODD3, 1030, 6, "far", "strided", "shared-1", {"msda_fwd_global": 1, "msda_bwd_global": 1}, ("bf16", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "SCATTER_MF"))),
    (2, 2, MSDA_T4, 129, 4, "border", "strided", "batch-1", {}, ("f32", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "SCATTER_LDS"))),
    (1, 8, MSDA_ODD4, 1041, 4, "spike", "dense", "batch-L+dref", {"msda_fwd_global": 1, "msda_bwd_global": 1}, ("bf16", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "ABSMAX", "SCATTER_MF"))),
    (2, 1, MSDA_ODD3, 1041, 4, "spike", "dense", "shared-1", {}, ("f32", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "ABSMAX", "SCATTER_LDS"))),
    (1, 8, ((2, 2), (2, 2), (1, 2)), 10, 4, "border", "dense", "shared-L+dref", {}, ("bf16", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "SCATTER_MF"))),
    (1, 8, ((16, 16),), 1041, 4, "centres", "dense", "shared-1+dref", {}, ("f32", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "ABSMAX", "SCATTER_LDS"))),
    (3, 4, ((7, 10),), 70, 4, "far", "strided", "batch-1", {"msda_fwd_global": 1, "msda_bwd_global": 1}, ("bf16", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "SCATTER_MF"))),
    (1, 8, ((40, 30),), None, 4, "ordinary", "strided", "shared-1", {}, ("f32", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "ABSMAX", "SCATTER_LDS"))),
    (1, 4, MSDA_ODD4, 1041, 4, "far", "strided", "batch-L", {}, ("f32", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "ABSMAX", "SCATTER_LDS"))),
    (2, 2, MSDA_MID3, 1041, 4, "lastquery", "dense", "batch-1", {"msda_fwd_global": 1, "msda_bwd_global": 1}, ("bf16", ("FWD_GLOBAL",), ("GRAD_GLOBAL", "ABSMAX", "SCATTER_MF"))),
    (1, 8, MSDA_ODD3, None, 4, "far", "dense", "shared-1", {"msda_fwd_global": 1}, ("f16", ("FWD_GLOBAL",), None)),
    (2, 4, MSDA_T4, 5, 4, "ordinary", "strided", "batch-L", {}, ("f16", ("FWD_GLOBAL",), None)),
    (1, 8, MSDA_FIN3, None, 6, "ordinary", "dense", "shared-1", {"msda_scatter_mfma": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_FIN3, None, 6, "spike", "strided", "shared-1", {"msda_scatter_mfma": 0, "msda_scatter_qsplit": 2}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_FIN3, None, 6, "far", "dense", "shared-L", {"msda_scatter_mfma": 0, "msda_scatter_qsplit": -1}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_LDS"))),
    (1, 8, MSDA_FIN3, None, 6, "ordinary", "strided", "batch-1", {"msda_scatter_mfma": 0, "msda_scatter_cuts": 3}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_LDS"))),
    (1, 8, MSDA_FIN4, None, 4, "border", "dense", "shared-1", {"msda_scatter_mfma": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_FIN4, None, 4, "spike", "strided", "shared-1", {"msda_scatter_mfma": 0, "msda_scatter_qsplit": 2}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_FIN3, None, 4, "ordinary", "dense", "shared-1", {"msda_scatter_mfma": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, MSDA_FIN3, None, 4, "far", "strided", "shared-1", {"msda_scatter_mfma": 0, "msda_scatter_qsplit": 2}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_LDS", "FINALIZE"))),
    (1, 8, ((32, 28),), 1041, 4, "spike", "dense", "shared-1", {"msda_scatter_mfma": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_LDS"))),
    (1, 8, ((32, 28),), 1041, 4, "lastquery", "strided", "shared-1", {"msda_scatter_mfma": 0, "msda_scatter_qsplit": 2}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_LDS"))),
    (2, 8, MSDA_MF3, None, 6, "ordinary", "dense", "shared-1", {"msda_scatter_mfma": 2, "msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (2, 8, MSDA_MF3, None, 6, "spike", "strided", "batch-1", {"msda_scatter_mfma": 2, "msda_lds_min_pairs": 0, "msda_mf_bands": 16}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (1, 8, MSDA_MF4, None, 4, "border", "dense", "shared-1", {"msda_scatter_mfma": 2, "msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (3, 4, MSDA_MF4, 113, 4, "lastquery", "strided", "shared-L", {"msda_scatter_mfma": 2, "msda_lds_min_pairs": 0, "msda_mf_bands": 16}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (1, 2, MSDA_MF3, None, 4, "far", "dense", "shared-1", {"msda_scatter_mfma": 2, "msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (2, 8, MSDA_MF3, 129, 4, "ordinary", "strided", "batch-L", {"msda_scatter_mfma": 2, "msda_lds_min_pairs": 0, "msda_mf_bands": 16}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (2, 8, ((7, 10),), None, 4, "border", "strided", "shared-1", {"msda_scatter_mfma": 2, "msda_lds_min_pairs": 0}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
    (1, 8, ((7, 10),), 129, 4, "spike", "dense", "shared-1", {"msda_scatter_mfma": 2, "msda_lds_min_pairs": 0, "msda_mf_bands": 16}, ("bf16", ("FWD_LDS",), ("GRAD_LDS", "SCATTER_MF"))),
)


def msda_cases(seed=2010):
    """(id, B, M, shapes, Lq or None, P, regime, layout, refmode, knobs, expect, seed); expect = (dtype, the kernel kinds the forward launches,
    those the backward launches or None for the forward-only float16) under the case's knobs, every other knob at its default"""
    return [("msda%d-%d" % (seed, i),) + row + (seed + i,) for i, row in enumerate(_MSDA_ROWS)]


def _msda_kinds(c):
    return set(c[10][1]) | set(c[10][2] or ())


def _msda_has(kind, build):
    return lambda c: kind in _msda_kinds(c) and (len(c[3]), c[5]) == build


def _msda_first_stage(c):
    return {k for k in _msda_kinds(c) if k.startswith(("FWD_", "GRAD_"))}


# FWD_BAND / GRAD_BAND need two levels; FINALIZE needs two levels cut differently (msda_ranges: a query split goes to the levels with fewer
# cuts than the most-cut one): none of the three exists for the (1, 4) build
MSDA_REGIMES = [("%s, build (%d, %d)" % (k, b[0], b[1]), _msda_has(k, b)) for k in MSDA_KINDS for b in MSDA_BUILDS
                if not (b[0] == 1 and k in ("FWD_BAND", "GRAD_BAND", "FINALIZE"))] + [
    ("band plan: NB = 4", lambda c: "FWD_BAND" in _msda_kinds(c) and msda_band_geometry(c[3], c[1], c[2], c[9].get("msda_band_halo", 0))[0] == 4),
    ("band plan: NB = 2", lambda c: "FWD_BAND" in _msda_kinds(c) and msda_band_geometry(c[3], c[1], c[2], c[9].get("msda_band_halo", 0))[0] == 2),
    ("band plan: msda_band_halo = 3 (misses)", lambda c: "FWD_BAND" in _msda_kinds(c) and c[9].get("msda_band_halo") == 3),
    ("Lq = 1", lambda c: c[4] == 1),
    ("Lq % 16 = 1, Lq > 1", lambda c: msda_lq(c) % 16 == 1 and msda_lq(c) > 1),
    ("Lq >= 1024 behind GRAD_GLOBAL (ABSMAX)", lambda c: msda_lq(c) >= 1024 and "ABSMAX" in _msda_kinds(c)),
    ("Lq >= 1024, no max |dout| scan (M = 3, 16)", lambda c: msda_lq(c) >= 1024 and "GRAD_GLOBAL" in _msda_kinds(c) and "ABSMAX" not in _msda_kinds(c)),
    ("fp32, Lq >= 1024", lambda c: c[10][0] == "f32" and msda_lq(c) >= 1024),
    ("fp32, a level cut into several scatter ranges", lambda c: c[10][0] == "f32" and any(h * w > msda_scatter_max_npix(c[3]) for h, w in c[3])),
    ("scatter ranges: msda_scatter_qsplit = 2", lambda c: c[9].get("msda_scatter_qsplit") == 2),
    ("scatter ranges: msda_scatter_qsplit = -1 or msda_scatter_cuts = 3", lambda c: c[9].get("msda_scatter_qsplit") == -1 or c[9].get("msda_scatter_cuts") == 3),
    ("matrix-product scatter: msda_mf_bands = 16", lambda c: c[9].get("msda_mf_bands") == 16 and "SCATTER_MF" in _msda_kinds(c)),
] + [("M = %d" % m, (lambda m_: lambda c: c[2] == m_)(m)) for m in (1, 2, 3, 4, 8, 16)] + [
    ("B = %d" % b, (lambda b_: lambda c: c[1] == b_)(b)) for b in (1, 2, 3)] + [
    ("dtype: %s" % d, (lambda d_: lambda c: c[10][0] == d_)(d)) for d in ("f32", "bf16", "f16")] + [
    ("inputs: %s" % r, (lambda r_: lambda c: c[6] == r_)(r)) for r in MSDA_INPUTS] + [
    ("strided, %s" % k, (lambda k_: lambda c: c[7] == "strided" and k_ in _msda_kinds(c))(k))
    for k in ("FWD_GLOBAL", "FWD_LDS", "FWD_BAND", "GRAD_GLOBAL", "GRAD_LDS", "GRAD_BAND", "SCATTER_MF", "SCATTER_LDS")] + [
    ("strided, band miss path", lambda c: c[7] == "strided" and "GRAD_BAND" in _msda_kinds(c) and (c[9].get("msda_band_halo") == 3 or c[6] in ("bandedge", "far"))),
] + [("refmode %s, %s" % (r, k), (lambda r_, k_: lambda c: c[8].partition("+")[0] == r_ and k_ in _msda_kinds(c))(r, k))
     for k in ("GRAD_GLOBAL", "GRAD_LDS", "GRAD_BAND") for r in MSDA_REFMODES] + [
    ("dref, GRAD_GLOBAL", lambda c: c[8].endswith("+dref") and "GRAD_GLOBAL" in _msda_kinds(c) and not c[9].get("msda_bwd_dref_lds", 1) == 0),
    ("dref, GRAD_LDS (msda_bwd_dref_lds = 1)", lambda c: c[8].endswith("+dref") and "GRAD_LDS" in _msda_kinds(c)),
    ("dref, msda_bwd_dref_lds = 0 (GRAD_GLOBAL)", lambda c: c[8].endswith("+dref") and c[9].get("msda_bwd_dref_lds", 1) == 0 and "GRAD_GLOBAL" in _msda_kinds(c)),
    ("dref on a band pyramid (GRAD_GLOBAL)", lambda c: c[8].endswith("+dref") and "FWD_BAND" in _msda_kinds(c) and "GRAD_GLOBAL" in _msda_kinds(c)),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# grouped 3x3 convolution: emrt_gconv2d / emrt_gconv2d_bwd (csrc/gconv.hip; tests/test_gpu_gconv_fuzz.py).  Written out like the msda list:
# every row ends with what it is there for, and the regimes are computed from the mirrored launch arithmetic below, not from that text.
# ---------------------------------------------------------------------------------------------------------------------------------
GCONV_LONG_MAX_ELEMS = 257 * 257 * 256          # per tensor, for the three grid-stride cases alone: the smallest maps that send a block round its tile loop twice
GCONV_DTYPES = ("f32", "bf16", "f16")
GCONV_EPILOGUES = ("none", "bias", "fold", "fold+relu", "stats", "stats+relu", "stats+bias")          # fold = scale + shift (eval-mode BatchNorm)
GCONV_VIEWS = ("dense", "ld", "bs", "ld+bs")          # ld: a channel slice of a wider buffer; bs: rows of padding behind every image
GCONV_ARMS = ("all", "dx", "dw", "dbias", "dx-acc+dw", "none")          # all = dx + dw + dbias in one call; none: the forward-only float16
GCONV_INPUTS = ("ordinary", "corner", "lastpixel")
GCONV_THREADS, GCONV_PPT = 256, 4          # GC_THREADS, GC_PPT


def gconv_block(quads):
    """(QB, PS): channel quads and pixel slots of a block.  Mirrors pick_block (csrc/gconv.hip)."""
    QB = quads if quads < 64 else 64
    return QB, GCONV_THREADS // QB


def gconv_grid(M, chans, stats):
    """(ntiles, gx, nslices, loops) of the forward over chans = OC output channels, or of the data gradient over chans = C input channels
    and M input pixels (stats False); loops: a block walks more than one pixel tile.  Mirrors launch_fwd / launch_dgrad (csrc/gconv.hip)."""
    quads = chans // 4
    QB, PS = gconv_block(quads)
    nslices = _ceil_div(quads, QB)
    ntiles = _ceil_div(M, PS * GCONV_PPT)
    cap = _ceil_div(2048, nslices) if stats else 4096
    gx = min(ntiles, cap)
    return ntiles, gx, nslices, ntiles > gx


def gconv_wgrad_plan(M, OC, Cg):
    """(threads, rows_per_slice, S): one thread per (oc, tap, 8- or 4-channel chunk), S slices of the pixel reduction over gridDim.y.
    Mirrors launch_wgrad (csrc/gconv.hip)."""
    CH = 8 if Cg >= 8 else 4
    threads = OC * 9 * (Cg // CH)
    S = max(1, min(1048576 // threads, M // 32))
    rows = _ceil_div(M, S)
    return threads, rows, _ceil_div(M, rows)


def gconv_view(kind, C, HW):
    """(ld, bs) of a tensor of C channels and HW pixels per image under a view kind of GCONV_VIEWS: ld = C rounded up to 8, plus 8; three
    pixel rows of padding behind each image"""
    ld = C if "ld" not in kind else (C + 7) // 8 * 8 + 8
    return ld, HW * ld + (3 * ld if "bs" in kind else 0)


def gconv_dims(case):
    """(C, OC, OH, OW, M forward = output pixels, M data gradient = input pixels)"""
    _, N, H, W, groups, Cg, Og, stride = case[:8]
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    return groups * Cg, groups * Og, OH, OW, N * OH * OW, N * H * W


def gconv_in_domain(case):
    """check_common plus the EMRT_REQUIRE lines of emrt_gconv2d and emrt_gconv2d_bwd (csrc/gconv.hip), under the strides gconv_view gives.  The
    input's ldin / in_bs (ldx / x_bs) must be multiples of 8, so an input with C % 8 != 0 (3 groups of 4) is legal only as a slice of a wider
    buffer (view `ld` or `ld+bs`); every other stride is a multiple of 4.  No statistics and no backward in float16."""
    _, N, H, W, groups, Cg, Og, stride, dtype, epilogue, views, arm, inputs, _, _ = case
    if not (N > 0 and H > 0 and W > 0 and groups > 0 and stride in (1, 2) and Cg in (4, 8, 16, 32) and Og > 0 and Og % 4 == 0):
        return False
    if dtype not in GCONV_DTYPES or epilogue not in GCONV_EPILOGUES or arm not in GCONV_ARMS or inputs not in GCONV_INPUTS:
        return False
    if len(views) != 4 or any(v not in GCONV_VIEWS for v in views) or N * H * W + 512 >= 2 ** 31:
        return False
    if dtype == "f16" and (arm != "none" or epilogue.startswith("stats")):
        return False
    if dtype != "f16" and arm == "none":
        return False
    C, OC, OH, OW, _, _ = gconv_dims(case)
    (ldin, in_bs), (ldout, out_bs) = gconv_view(views[0], C, H * W), gconv_view(views[1], OC, OH * OW)
    (lddy, dy_bs), (lddx, dx_bs) = gconv_view(views[2], OC, OH * OW), gconv_view(views[3], C, H * W)
    return (ldin >= C and in_bs >= H * W * ldin and ldin % 8 == 0 and in_bs % 8 == 0
            and ldout >= OC and out_bs >= OH * OW * ldout and ldout % 4 == 0 and out_bs % 4 == 0
            and lddy >= OC and dy_bs >= OH * OW * lddy and lddy % 4 == 0 and dy_bs % 4 == 0
            and lddx >= C and dx_bs >= H * W * lddx and lddx % 4 == 0 and dx_bs % 4 == 0)


_D = "dense"
_DENSE = (_D, _D, _D, _D)
# (N, H, W, groups, Cg, Og, stride, dtype, epilogue, views of (input, output, dy, dx), backward arm, input recipe, what the row is there for)
_GCONV_ROWS = (
    (2, 9, 7, 3, 4, 4, 1, "f32", "none", ("ld", _D, _D, _D), "all", "ordinary", "3 groups of 4: C = 12 only as a slice, QB = 3 both ways (85 slots, one idle thread), M below a tile"),
    (2, 9, 7, 3, 4, 12, 1, "bf16", "bias", ("ld+bs", "ld", _D, "bs"), "all", "ordinary", "Og 12 > Cg 4: 9 output quads (QB = 9, 28 slots, 4 idle threads)"),
    (1, 17, 13, 5, 4, 4, 2, "bf16", "none", ("ld", "bs", "ld", _D), "dx", "ordinary", "5 groups, stride 2 on odd sizes, dx alone"),
    (2, 6, 10, 6, 4, 20, 2, "f32", "fold", ("ld+bs", _D, "bs", "ld"), "dw", "ordinary", "Og 20, stride 2 on even sizes, M = 30 (S = 1), dw alone, a ragged last wgrad block"),
    (2, 5, 11, 4, 8, 4, 1, "f32", "stats", (_D, "ld", _D, "ld+bs"), "all", "ordinary", "Og 4 < Cg 8; QB = 4: 64 pixel slots in the statistics' column sum"),
    (1, 12, 12, 8, 8, 8, 1, "bf16", "stats", _DENSE, "dx-acc+dw", "ordinary", "all dense, dx accumulates onto what is there"),
    (3, 7, 5, 2, 8, 12, 1, "bf16", "stats+bias", ("bs", "ld+bs", "ld+bs", _D), "dbias", "ordinary", "Og 12 > Cg 8, dbias alone, 35 pixels per image: a thread's pixels cross image ends"),
    (1, 8, 8, 6, 8, 4, 2, "f32", "fold+relu", ("ld", "bs", _D, "bs"), "dx", "ordinary", "Og 4, 12 input quads and 6 output quads (neither divides 256), stride 2 on even sizes"),
    (2, 4, 6, 4, 16, 16, 1, "f32", "bias", ("bs", _D, "ld", "ld"), "all", "ordinary", "Cg 16 fp32: two 8-channel passes per tap"),
    (1, 10, 3, 2, 16, 4, 1, "bf16", "none", (_D, "ld+bs", "bs", "ld+bs"), "dx-acc+dw", "ordinary", "Og 4 < Cg 16: 2 output quads, 128 pixel slots; M = 30 far below the 512-pixel tile"),
    (2, 3, 9, 5, 16, 20, 2, "bf16", "fold", ("ld", "ld", _D, _D), "dw", "ordinary", "Og 20 > Cg 16, 20 input and 25 output quads, stride 2 (odd sizes), dw alone"),
    (1, 1, 13, 3, 16, 8, 1, "f32", "stats+relu", (_D, _D, "ld", "bs"), "all", "ordinary", "H = 1: only the middle kernel row is ever inside"),
    (1, 6, 6, 2, 32, 32, 1, "f32", "none", ("ld+bs", "ld", "ld+bs", "ld+bs"), "dx", "ordinary", "Cg 32 fp32: four passes per tap, every tensor a padded view"),
    (2, 2, 5, 8, 32, 32, 1, "bf16", "bias", _DENSE, "all", "ordinary", "C = OC = 256: exactly one full slice both ways; H = 2"),
    (1, 7, 2, 10, 32, 8, 2, "bf16", "none", ("bs", "bs", "ld", "ld"), "all", "ordinary", "C = 320: 80 input quads, the data gradient's second slice is ragged; W = 2 under stride 2"),
    (1, 5, 1, 3, 32, 12, 1, "f32", "stats+bias", (_D, "ld+bs", "bs", _D), "all", "ordinary", "W = 1; Og 12 < Cg 32"),
    (1, 9, 9, 16, 4, 20, 1, "bf16", "stats", (_D, "ld", _D, "ld"), "all", "ordinary", "OC = 320: the forward's second slice is ragged, with statistics (oc < OC in the column sum)"),
    (2, 5, 4, 10, 8, 32, 1, "f32", "bias", ("ld", "bs", "ld+bs", "bs"), "all", "ordinary", "OC = 320 again in fp32, 20 input quads"),
    (1, 4, 4, 16, 4, 16, 1, "bf16", "fold+relu", (_D, _D, _D, _D), "dx", "ordinary", "OC = 256: one full forward slice from 16 input quads"),
    (1, 3, 5, 32, 8, 4, 1, "f32", "none", (_D, "ld", "ld", "bs"), "dx-acc+dw", "ordinary", "C = 256: one full data-gradient slice; 32 output quads"),
    (2, 2, 2, 20, 16, 4, 1, "bf16", "stats", ("ld", _D, "bs", "ld+bs"), "all", "ordinary", "C = 320 from 20 groups of 16; a 2 x 2 map: every tap position is a border"),
    (2, 3, 3, 4, 4, 4, 1, "bf16", "stats+relu", (_D, "bs", "ld", _D), "dbias", "ordinary", "ReLU together with statistics in bf16, dbias alone"),
    (2, 13, 17, 2, 4, 8, 1, "f32", "fold", ("bs", "ld+bs", "ld", "ld"), "all", "ordinary", "M = 442: two 256-pixel tiles, the second ragged; 13 wgrad slices of 34 rows"),
    (1, 13, 17, 8, 4, 4, 1, "bf16", "stats+bias", (_D, _D, "ld+bs", "bs"), "all", "ordinary", "OC = 32: 288 wgrad threads (a ragged second block), 6 slices of 37 rows"),
    (3, 11, 6, 2, 16, 16, 2, "f32", "stats+relu", ("ld", "ld", "bs", "ld"), "dw", "ordinary", "stride 2 on an odd and an even size at once, 18 pixels per image"),
    (2, 16, 10, 4, 32, 4, 2, "bf16", "fold+relu", ("ld+bs", _D, _D, "ld+bs"), "dx", "ordinary", "Og 4 < Cg 32, stride 2 on even sizes"),
    (2, 6, 7, 4, 4, 8, 1, "f32", "none", ("ld", "ld", "ld", "ld"), "all", "corner", "corner pixels only: a halo or bounds slip changes an exact, small set"),
    (1, 9, 5, 2, 16, 16, 2, "bf16", "bias", ("bs", "bs", "bs", "bs"), "all", "corner", "corner pixels under stride 2"),
    (2, 5, 3, 3, 8, 12, 1, "bf16", "none", (_D, "ld+bs", "ld+bs", "ld+bs"), "dx", "corner", "corner pixels, Og 12, dx alone"),
    (2, 7, 6, 4, 8, 8, 1, "bf16", "none", ("ld+bs", _D, "ld", "bs"), "all", "lastpixel", "dy at the last output pixel alone"),
    (1, 8, 11, 3, 4, 4, 2, "f32", "none", ("ld", _D, _D, _D), "all", "lastpixel", "dy at the last output pixel under stride 2, C = 12"),
    (3, 5, 5, 2, 32, 20, 1, "f32", "none", (_D, _D, "bs", "ld"), "dbias", "lastpixel", "dbias of one pixel: every other channel sum is an exact zero"),
    (2, 9, 14, 8, 4, 4, 1, "f16", "none", ("ld", "ld", _D, _D), "none", "ordinary", "fp16 forward at Cg 4"),
    (1, 7, 5, 4, 8, 12, 2, "f16", "bias", ("bs", "bs", _D, _D), "none", "ordinary", "fp16 forward at Cg 8 with bias, stride 2"),
    (2, 6, 6, 2, 32, 8, 1, "f16", "fold+relu", (_D, "ld+bs", _D, _D), "none", "ordinary", "fp16 forward at Cg 32, folded BatchNorm + ReLU"),
    (1, 5, 9, 3, 8, 8, 1, "f16", "none", ("ld+bs", _D, _D, _D), "none", "ordinary", "fp16 forward at Cg 8, 6 quads"),
    (2, 4, 3, 2, 32, 32, 2, "f16", "bias", ("ld", "ld", _D, _D), "none", "ordinary", "fp16 forward at Cg 32 with bias"),
    (1, 11, 6, 6, 4, 8, 1, "f16", "fold+relu", (_D, "bs", _D, _D), "none", "ordinary", "fp16 forward at Cg 4, folded BatchNorm + ReLU"),
    (1, 257, 257, 8, 4, 32, 1, "bf16", "none", _DENSE, "all", "ordinary", "4129 forward tiles on 4096 blocks: the forward's grid-stride loop"),
    (1, 257, 257, 8, 32, 4, 1, "bf16", "bias", _DENSE, "all", "ordinary", "4129 data-gradient tiles on 4096 blocks: the data gradient's grid-stride loop"),
    (1, 65, 65, 16, 4, 128, 1, "f32", "stats", _DENSE, "all", "ordinary", "265 tiles on 256 blocks x 8 slices: statistics summed over two tiles per thread; S = 56 bounded by the thread count"),
)


def gconv_cases(seed=2111):
    """(id, N, H, W, groups, Cg, Og, stride, dtype, epilogue, views, arm, inputs, why, seed)"""
    return [("gconv%d-%d" % (seed, i),) + row + (seed + i,) for i, row in enumerate(_GCONV_ROWS)]


def _gc_has_dx(c):
    return c[11] in ("all", "dx", "dx-acc+dw")


def _gc_has_wgrad(c):
    return c[11] in ("all", "dw", "dbias", "dx-acc+dw")


def _gc_fwd_quads(c):
    return gconv_dims(c)[1] // 4


def _gc_dgrad_quads(c):
    return gconv_dims(c)[0] // 4 if _gc_has_dx(c) else None


def _gc_block_regimes(side, quads_of):
    return [
        ("%s: QB < 64 dividing 256" % side, lambda c: quads_of(c) is not None and quads_of(c) < 64 and 256 % quads_of(c) == 0),
        ("%s: QB not dividing 256 (idle threads)" % side, lambda c: quads_of(c) is not None and quads_of(c) < 64 and 256 % quads_of(c) != 0),
        ("%s: exactly one full slice" % side, lambda c: quads_of(c) == 64),
        ("%s: several slices, ragged last" % side, lambda c: quads_of(c) is not None and quads_of(c) > 64 and quads_of(c) % 64 != 0),
    ]


def _gc_fwd_tile(c):
    return GCONV_PPT * gconv_block(_gc_fwd_quads(c))[1]


def _gc_fwd_grid(c):
    return gconv_grid(gconv_dims(c)[4], gconv_dims(c)[1], c[9].startswith("stats"))


def _gc_plan(c):
    return gconv_wgrad_plan(gconv_dims(c)[4], gconv_dims(c)[1], c[5]) if _gc_has_wgrad(c) else None


GCONV_REGIMES = [("Cg = %d, %s" % (cg, d), (lambda cg_, d_: lambda c: c[5] == cg_ and c[8] == d_)(cg, d)) for cg in (4, 8, 16, 32) for d in ("f32", "bf16")] + [
    ("Og == Cg", lambda c: c[6] == c[5]),
    ("Og < Cg", lambda c: c[6] < c[5]),
    ("Og > Cg", lambda c: c[6] > c[5]),
    ("Og = 4", lambda c: c[6] == 4),
    ("Og not a power of two (12, 20)", lambda c: c[6] in (12, 20)),
] + _gc_block_regimes("forward", _gc_fwd_quads) + _gc_block_regimes("dgrad", _gc_dgrad_quads) + [
    ("forward: M below one tile", lambda c: gconv_dims(c)[4] < _gc_fwd_tile(c)),
    ("forward: M % (4 PS) != 0", lambda c: gconv_dims(c)[4] % _gc_fwd_tile(c) != 0),
    ("forward: M % 4 != 0", lambda c: gconv_dims(c)[4] % 4 != 0),
    ("forward: OW % 4 != 0 (pixels cross a row end)", lambda c: gconv_dims(c)[3] % 4 != 0),
    ("forward: N > 1, OH OW % 4 != 0 (pixels cross an image end)", lambda c: c[1] > 1 and (gconv_dims(c)[2] * gconv_dims(c)[3]) % 4 != 0),
    ("dgrad: W % 4 != 0 (pixels cross a row end)", lambda c: _gc_has_dx(c) and c[3] % 4 != 0),
    ("dgrad: N > 1, H W % 4 != 0 (pixels cross an image end)", lambda c: _gc_has_dx(c) and c[1] > 1 and (c[2] * c[3]) % 4 != 0),
    ("grid-stride: forward, no statistics", lambda c: not c[9].startswith("stats") and _gc_fwd_grid(c)[3]),
    ("grid-stride: forward with statistics", lambda c: c[9].startswith("stats") and _gc_fwd_grid(c)[3]),
    ("grid-stride: dgrad", lambda c: _gc_has_dx(c) and gconv_grid(gconv_dims(c)[5], gconv_dims(c)[0], False)[3]),
    ("stride 1", lambda c: c[7] == 1),
    ("stride 2", lambda c: c[7] == 2),
    ("H or W = 1", lambda c: 1 in (c[2], c[3])),
    ("H or W = 2", lambda c: 2 in (c[2], c[3])),
    ("stride 2 on an even size", lambda c: c[7] == 2 and (c[2] % 2 == 0 or c[3] % 2 == 0)),
    ("stride 2 on an odd size", lambda c: c[7] == 2 and (c[2] % 2 == 1 or c[3] % 2 == 1)),
    ("non-square", lambda c: c[2] != c[3]),
] + [("%s view: %s" % (t, v), (lambda i_, v_, need_: lambda c: c[10][i_] == v_ and need_(c))(i, v, need))
     for i, (t, need) in enumerate((("input", lambda c: True), ("output", lambda c: True), ("dy", lambda c: c[11] != "none"), ("dx", _gc_has_dx)))
     for v in ("ld", "bs", "ld+bs")] + [
    ("all dense", lambda c: c[10] == _DENSE),
] + [("epilogue: %s" % e, (lambda e_: lambda c: c[9] == e_)(e)) for e in GCONV_EPILOGUES] + [
    ("f16 epilogue: %s" % e, (lambda e_: lambda c: c[8] == "f16" and c[9] == e_)(e)) for e in ("none", "bias", "fold+relu")] + [
    ("f16 at Cg = %d" % cg, (lambda cg_: lambda c: c[8] == "f16" and c[5] == cg_)(cg)) for cg in (4, 8, 32)] + [
    ("backward arm: %s" % a, (lambda a_: lambda c: c[11] == a_)(a)) for a in GCONV_ARMS] + [
    ("wgrad: S = 1", lambda c: _gc_plan(c) is not None and _gc_plan(c)[2] == 1),
    ("wgrad: S > 1, rows_per_slice % 4 != 0", lambda c: _gc_plan(c) is not None and _gc_plan(c)[2] > 1 and _gc_plan(c)[1] % 4 != 0),
    ("wgrad: S bounded by the thread count", lambda c: _gc_plan(c) is not None and 1048576 // _gc_plan(c)[0] < gconv_dims(c)[4] // 32),
    ("wgrad: threads % 256 != 0", lambda c: _gc_plan(c) is not None and _gc_plan(c)[0] % 256 != 0),
] + [("inputs: %s" % r, (lambda r_: lambda c: c[12] == r_)(r)) for r in GCONV_INPUTS]


# ---------------------------------------------------------------------------------------------------------------------------------
# dense convolution, the fused epilogues: emrt_conv2d (mode 0) / emrt_conv2d_bwd / emrt_conv2d_dgrad_multi / emrt_conv2d_group (csrc/conv.hip,
# csrc/igemm8p.hpp; tests/test_gpu_conv_epilogue_fuzz.py).  Written out like the gconv list; the host-side decisions of conv.hip are restated
# below as pure functions of a case, and the regimes -- (kernel kind) x (epilogue copy) x (epilogue features) -- are computed from them.
# ---------------------------------------------------------------------------------------------------------------------------------
CONV_ESZ = {"f32": 4, "bf16": 2, "f16": 2}
CONV_FWD_EPILOGUES = ("none", "bias", "fold", "residual", "relu", "stats", "out_f32", "bias+residual+relu", "fold+relu", "stats+relu", "out_f32+bias")
# mask: zero where mask_y <= 0; maskx: mask_y is x itself (the thin kernel's MASK = 1); scale: mask_scale = 1 / (1 - 0.25)
CONV_BWD_EPILOGUES = ("none", "stats", "mask", "mask+stats", "mask+stats+stat_x", "mask+scale", "addend", "addend+mask+stats+stat_x", "accumulate",
                      "accumulate+mask+stats", "accumulate+stats", "maskx", "maskx+stats")
CONV_ARMS = ("dx", "dx+dw", "dx+dw+dbias")
CONV_ROLES = {"fwd": ("in", "out", "res"), "bwd": ("x", "dy", "dx", "mask", "statx", "addend")}
CONV_VIEWS = ("ld", "bs", "ld+bs")
CONV_INPUTS = ("ordinary", "corner", "lastpixel")
# the tuning knobs a case may set, with the library's defaults (csrc/elementwise.hip)
CONV_KNOBS = dict(conv_tile=0, xk=0, pair_max=768, no_s2_dgrad=0, no_thin_bwd=0, no_ksplit128=0, igemm8p_cmajor=0, igemm8p_min_blocks=160, no_bna=0,
                  thin_cblk=64, thin_blocks=128, thin_ch=8, wgrad_split=0)
CONV_KINDS = ("64x64 G1", "64x64 G2", "64x64 G4", "128x64", "128x128 G1", "128x128 G2", "256x32", "xk", "s2", "8p", "pair", "thin")
CONV_TILE = {"64x64": (64, 64), "128x64": (128, 64), "128x128": (128, 128), "256x32": (256, 32), "xk": (64, 64), "s2": (64, 64), "8p": (256, 256),
             "pair": (64, 64)}


class _NS(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def conv_case_fields(c):
    """a case as a namespace: (id, N, H, W, C, OC, k, stride, pad, dil, dtype, side, epilogue, arm, views, knobs, twin, inputs, why, seed)"""
    keys = ("id", "N", "H", "W", "C", "OC", "k", "stride", "pad", "dil", "dtype", "side", "epilogue", "arm", "views", "knobs", "twin", "inputs", "why", "seed")
    return _NS(**dict(zip(keys, c)))


def conv_out_size(S, k, stride, pad, dil):
    return (S + 2 * pad - dil * (k - 1) - 1) // stride + 1


def conv_feats(c):
    """the epilogue's features as a set: fold = scale + bias; mask+scale = mask + mask_scale; maskx = mask whose tensor is x"""
    toks = set(c[12].split("+")) - {"none"}
    if "fold" in toks:
        toks = (toks - {"fold"}) | {"scale", "bias"}
    if c[11] == "bwd" and "scale" in toks:
        toks = (toks - {"scale"}) | {"mask_scale"}
    if "maskx" in toks:
        toks = (toks - {"maskx"}) | {"mask", "mask_is_x"}
    return frozenset(toks)


def conv_parse_views(spec, roles):
    """'mask:ld8 dx:ld+bs' -> {role: (kind, channel offset)}; a role the string does not name is dense"""
    out = dict((r, ("dense", 0)) for r in roles)
    for tok in spec.split():
        role, _, v = tok.partition(":")
        kind = v.rstrip("0123456789")
        if role not in out or kind not in CONV_VIEWS:
            raise ValueError("bad view %r" % tok)
        out[role] = (kind, int(v[len(kind):] or 0))
    return out


def conv_view(kind, off, ch, pix):
    """(ld, bs) of a tensor of ch channels and pix pixels per image: `ld` makes it the channels [off, off + ch) of a buffer of ch + off rounded up
    to 8, plus 8, channels (the offset decides the 16-byte alignment of the slice); `bs` puts three pixel rows of padding behind every image"""
    ld = ch if "ld" not in kind else (ch + off + 7) // 8 * 8 + 8
    return ld, pix * ld + (3 * ld if "bs" in kind else 0)


def conv_tensors(c):
    """{role: namespace(ch, pix, ld, bs, off, esz, al)} of the tensors the call takes (al: the slice starts on a 16-byte boundary)"""
    f = conv_case_fields(c)
    OH, OW = conv_out_size(f.H, f.k, f.stride, f.pad, f.dil), conv_out_size(f.W, f.k, f.stride, f.pad, f.dil)
    feats, esz = conv_feats(c), CONV_ESZ[f.dtype]
    views = conv_parse_views(f.views, CONV_ROLES[f.side])
    if f.side == "fwd":
        geo = {"in": (f.C, f.H * f.W, esz, True), "out": (f.OC, OH * OW, 4 if "out_f32" in feats else esz, True), "res": (f.OC, OH * OW, esz, "residual" in feats)}
    else:
        px = f.H * f.W
        geo = {"x": (f.C, px, esz, True), "dy": (f.OC, OH * OW, esz, True), "dx": (f.C, px, esz, True),
               "mask": (f.C, px, esz, "mask" in feats and "mask_is_x" not in feats), "statx": (f.C, px, esz, "stat_x" in feats), "addend": (f.C, px, esz, "addend" in feats)}
    out = {}
    for role, (ch, pix, e, present) in geo.items():
        kind, off = views[role]
        if not present:
            if kind != "dense":
                raise ValueError("%s: a view for %s, which the call does not take" % (f.id, role))
            continue
        ld, bs = conv_view(kind, off, ch, pix)
        out[role] = _NS(ch=ch, pix=pix, ld=ld, bs=bs, off=off if "ld" in kind else 0, esz=e, al=((off if "ld" in kind else 0) * e) % 16 == 0, kind=kind)
    if f.side == "bwd" and "mask_is_x" in feats:
        out["mask"] = out["x"]
    return out


def conv_problem(c, knobs=None):
    """(a, w): the ConvArgs the entry point builds (conv_fwd_args / conv_dgrad_args: the data gradient is the swapped convolution, in = dy, out = dx)
    and the WgradArgs (None without dw).  Pointers appear as their 16-byte alignment; the packed weights are aligned."""
    f = conv_case_fields(c)
    kn = conv_knobs(c) if knobs is None else knobs
    OH, OW = conv_out_size(f.H, f.k, f.stride, f.pad, f.dil), conv_out_size(f.W, f.k, f.stride, f.pad, f.dil)
    feats, t, esz = conv_feats(c), conv_tensors(c), CONV_ESZ[f.dtype]
    a = _NS(esz=esz, KH=f.k, KW=f.k, stride=f.stride, pad=f.pad, dil=f.dil, N=f.N, cmajor=kn["igemm8p_cmajor"], stats="stats" in feats,
            res=False, ldres=0, res_bs=0, res_al=True, res_is_out=False, mask=False, ldy=0, y_bs=0, mask_al=True, mask_is_x=False,
            statx=False, ldsx=0, sx_bs=0, sx_al=True, bias=False, scale=False, relu=False, out_f32=False)
    if f.side == "fwd":
        a.mode, a.H, a.W, a.C, a.OH, a.OW, a.OC = 0, f.H, f.W, f.C, OH, OW, f.OC
        a.ldin, a.in_bs, a.in_al = t["in"].ld, t["in"].bs, t["in"].al
        a.ldout, a.out_bs, a.out_al = t["out"].ld, t["out"].bs, t["out"].al
        a.bias, a.scale, a.relu, a.out_f32 = "bias" in feats, "scale" in feats, "relu" in feats, "out_f32" in feats
        if "residual" in feats:
            a.res, a.ldres, a.res_bs, a.res_al = True, t["res"].ld, t["res"].bs, t["res"].al
        return a, None
    a.mode, a.H, a.W, a.C, a.OH, a.OW, a.OC = 1, OH, OW, f.OC, f.H, f.W, f.C
    a.ldin, a.in_bs, a.in_al = t["dy"].ld, t["dy"].bs, t["dy"].al
    a.ldout, a.out_bs, a.out_al = t["dx"].ld, t["dx"].bs, t["dx"].al
    if "accumulate" in feats:
        a.res, a.ldres, a.res_bs, a.res_al, a.res_is_out = True, a.ldout, a.out_bs, a.out_al, True
    elif "addend" in feats:
        a.res, a.ldres, a.res_bs, a.res_al = True, t["addend"].ld, t["addend"].bs, t["addend"].al
    if "mask" in feats:
        a.mask, a.ldy, a.y_bs, a.mask_al, a.mask_is_x = True, t["mask"].ld, t["mask"].bs, t["mask"].al, "mask_is_x" in feats
    if "stat_x" in feats:
        a.statx, a.ldsx, a.sx_bs, a.sx_al = True, t["statx"].ld, t["statx"].bs, t["statx"].al
    w = None
    if "dw" in f.arm:
        w = _NS(esz=esz, N=f.N, H=f.H, W=f.W, C=f.C, ldx=t["x"].ld, x_bs=t["x"].bs, x_al=t["x"].al, OH=OH, OW=OW, OC=f.OC, lddy=t["dy"].ld, dy_bs=t["dy"].bs,
                dy_al=t["dy"].al, KH=f.k, KW=f.k, stride=f.stride, pad=f.pad, dil=f.dil, dbias="dbias" in f.arm)
    return a, w


def conv_knobs(c, twin=False):
    """the knob values a case's launch runs under: CONV_KNOBS overridden by the case's own (or its twin's) set"""
    kn = dict(CONV_KNOBS)
    kn.update(dict(c[16] if twin else c[15]))
    return kn


# ---- csrc/conv.hip, host side ----------------------------------------------------------------------------------------------------
def conv_is_vec(a):
    """Mirrors conv_is_vec: C in whole 16-byte chunks, rows and images of `in` 16-byte aligned (the packed weight always is)"""
    epc = 16 // a.esz
    return a.C % epc == 0 and a.ldin % epc == 0 and a.in_bs % epc == 0 and a.in_al


def conv_blocks(a, bm, bn):
    return _ceil_div(a.N * a.OH * a.OW, bm) * _ceil_div(a.OC, bn)


def conv_k_tiles(a):
    return _ceil_div(a.KH * a.KW * a.C, 8 * (16 // a.esz))


def conv_takes_128(a):
    return a.OC > 64 and conv_k_tiles(a) >= 16 and conv_blocks(a, 128, 128) >= 256


def _conv_epi_aligned(a):
    """what igemm_s2_ok, igemm_xk_copies and the row-vectorised epilogue all ask of the epilogue operands but for OC % 8 and the output's own rows"""
    epc = 16 // a.esz
    return (a.out_al and (not a.res or a.res_al) and (not a.mask or a.mask_al) and (not a.statx or a.sx_al)
            and (not a.res or (a.ldres % epc == 0 and a.res_bs % epc == 0)) and (not a.mask or (a.ldy % epc == 0 and a.y_bs % epc == 0))
            and (not a.statx or (a.ldsx % epc == 0 and a.sx_bs % epc == 0)))


def conv_epilogue_vec_ok(a):
    """Mirrors vec_ok of igemm_body's epilogue: true = the row-vectorised copy, false = the scalar one"""
    eo = 4 if a.out_f32 else 16 // a.esz
    return _conv_epi_aligned(a) and a.ldout % eo == 0 and a.out_bs % eo == 0 and a.OC % 8 == 0


def igemm_s2_ok(a, kn):
    """Mirrors igemm_s2_ok: the parity-class kernel for the data gradient of a stride-2 convolution"""
    epc = 16 // a.esz
    M = a.N * a.OH * a.OW
    if a.KH * a.KW == 1 and kn["no_s2_dgrad"] != -1:
        return False
    if (kn["no_s2_dgrad"] == 1 or a.stride != 2 or a.dil != 1 or a.C % (8 * epc) != 0 or a.OH & 1 or a.OW & 1 or M % 4 or (M // 4) % 64 or a.OC <= 32
            or a.OC % 8):
        return False
    if a.out_f32 or a.bias or a.scale:
        return False
    return _conv_epi_aligned(a) and a.ldout % epc == 0 and a.out_bs % epc == 0


def igemm_xk_copies(a, kn, scratch):
    """Mirrors igemm_xk_copies: copies of the 64x64 tile grid the K range is cut over, 0 = not applicable.  scratch: the partial-tile region is
    registered on the launching stream (tests.hip_utils.init does that for the 2-byte dtypes); the 8 MiB / 16384-counter limits are mirrored"""
    if a.esz != 2 or kn["xk"] < 0 or not scratch:
        return 0
    if a.OC <= 32 or a.OC % 8 or a.out_f32:
        return 0
    if not (_conv_epi_aligned(a) and a.ldout % 8 == 0 and a.out_bs % 8 == 0):
        return 0
    nb, nkt = conv_blocks(a, 64, 64), conv_k_tiles(a)
    S = kn["xk"] if kn["xk"] > 0 else 0
    if S <= 0:
        if not ((nb <= 64 and nkt >= 36) or (nb <= 128 and nkt >= 128)):
            return 0
        S = 4
    S = min(S, nkt)
    if S >= 2:
        per = _ceil_div(nkt, S)
        S = _ceil_div(nkt, per)
    if S < 2 or nb > 16384 or nb * S * 64 * 64 * 4 > (8 << 20):
        return 0
    return S


def igemm8p_ok(a):
    """Mirrors igemm8p_ok (csrc/igemm8p.hpp): the 256x256 LDS-DMA kernel's operand and epilogue conditions"""
    if a.esz != 2 or a.C % 64 or a.OC % 8:
        return False
    if a.ldin % 8 or a.in_bs % 8 or not a.in_al:
        return False
    eo = 4 if a.out_f32 else 8
    if not a.out_al or a.ldout % eo or a.out_bs % eo:
        return False
    if a.res and (not a.res_al or a.ldres % 8 or a.res_bs % 8):
        return False
    if a.mask and (not a.mask_al or a.ldy % 8 or a.y_bs % 8):
        return False
    return not (a.statx and (not a.sx_al or a.ldsx % 8 or a.sx_bs % 8))


def conv_plan(a, kn, scratch):
    """(kind, n, forced): mirrors conv_plan<T, MODE, VEC> without the dropout epilogue (emrt_conv2d_drop is not swept here).  kind: 64x64,
    128x64, 128x128, 256x32, xk, s2, 8p; n: wave groups (64x64, 128x128) or copies (xk).  A forced tile the layer cannot take falls through the
    ladder below it, minus the cross-block split."""
    vec = conv_is_vec(a)
    vec2 = vec and a.esz == 2
    tile = kn["conv_tile"]
    if a.mode == 1 and vec and not tile and igemm_s2_ok(a, kn):
        return "s2", 1, False
    if tile == 1:
        return "64x64", 1, True
    if tile == 2:
        return "128x64", 1, True
    if tile == 3:
        return "128x128", 1, True
    if tile == 4:
        return "256x32", 1, True
    if tile == 5 and vec:
        return "64x64", 2, True
    if tile == 6 and vec:
        return "64x64", 4, True
    if tile == 7 and vec2 and igemm8p_ok(a):
        return "8p", 1, True
    if tile == 8 and vec2:
        return "128x128", 2, True
    if a.OC <= 32:
        return "256x32", 1, False
    if vec2 and not tile:
        S = igemm_xk_copies(a, kn, scratch)
        if S >= 2:
            return "xk", S, False
    if vec2:
        nb256, nkt64, minb = conv_blocks(a, 256, 256), a.KH * a.KW * a.C // 64, kn["igemm8p_min_blocks"]
        if minb > 0 and nkt64 >= 16 and (nb256 >= minb or (nb256 >= (minb * 3) // 5 and nkt64 >= 144)) and igemm8p_ok(a):
            return "8p", 1, False
    nkt = conv_k_tiles(a)
    if conv_takes_128(a):
        ksplit = vec2 and nkt >= 32 and conv_blocks(a, 128, 128) == 256 and not kn["no_ksplit128"]
        return "128x128", 2 if ksplit else 1, False
    if vec:
        nb = conv_blocks(a, 64, 64)
        if nb <= 128 and nkt >= 32:
            return "64x64", 4, False
        if nb <= 256 and nkt >= 16:
            return "64x64", 2, False
    return "64x64", 1, False


def bna_plan(a, kn, scratch):
    """Mirrors bna_plan: the kind that runs the layer with the BatchNorm on its A operand, or "none" (a_out aligned)"""
    bk = 8 * (16 // a.esz)
    if not conv_is_vec(a) or a.C % bk or a.C > 1024 or a.OC <= 32:
        return "none", 0, False
    if a.stride != 1 or a.KH != a.KW or a.KH not in (1, 3) or a.pad != a.dil * (a.KH >> 1) or a.OH != a.H or a.OW != a.W:
        return "none", 0, False
    if a.KH == 3 and a.C > 128 and kn["no_bna"] != -1:
        return "none", 0, False
    p = conv_plan(a, kn, scratch)
    if kn["conv_tile"] and not p[2]:
        return "none", 0, False
    return p if p[0] in ("64x64", "xk") else ("none", 0, False)


def wgrad_is_vec(w):
    epc = 16 // w.esz
    return w.C % epc == 0 and w.OC % epc == 0 and w.ldx % epc == 0 and w.lddy % epc == 0 and w.x_bs % epc == 0 and w.dy_bs % epc == 0 and w.x_al and w.dy_al


def wgrad_plan(w, kn):
    """(tx, ty, S): mirrors wgrad_plan's cost model (the same double arithmetic)"""
    bkm = 64 if w.esz == 2 else 32
    K, M = w.KH * w.KW * w.C, w.N * w.OH * w.OW
    tx, ty = _ceil_div(K, 128), _ceil_div(w.OC, 128)
    mt = _ceil_div(M, bkm)
    atom_us = float(tx) * 128.0 * float(ty) * 128.0 * 4.0 / 1.3e6
    S, best = 1, 1e30
    for sc in (1, 2, 4, 8, 16, 32, 64, 128):
        if sc > mt or (sc > 1 and tx * ty >= 256):
            break
        per, nblk = float(_ceil_div(mt, sc)), float(tx) * ty * sc
        t = per * (nblk / 1024.0 if nblk > 1024.0 else 1.0) + sc * atom_us
        if t < best:
            best, S = t, sc
    if kn["wgrad_split"] > 0:
        S = min(kn["wgrad_split"], mt)
    per = _ceil_div(mt, S)
    return tx, ty, _ceil_div(mt, per)


def thin_bwd_ok(a, w):
    """Mirrors thin_bwd_ok: the one-pass backward of a 1x1 layer with at most 8 output channels (the 2^31-element limits hold for every case here)"""
    if w is None or w.KH != 1 or w.KW != 1 or w.stride != 1 or w.pad != 0 or w.OC > 8:
        return False
    if a.statx or (a.res and a.mask) or (a.res and not a.res_is_out):
        return False
    if w.C < 32 or w.C > 1024 or w.C & (w.C - 1):
        return False
    if not w.x_al or not a.out_al or (a.mask and not a.mask_al):
        return False
    if w.ldx % 4 or w.x_bs % 4 or a.ldout % 4 or a.out_bs % 4:
        return False
    return not (a.mask and (a.ldy % 4 or a.y_bs % 4))


def thin_bwd_geometry(a, w, kn):
    """(CH, pixel slots per block, pixels per block, MASK): mirrors thin_bwd_launch / thin_bwd_launch_ch"""
    can8 = w.C >= 64 and w.ldx % 8 == 0 and w.x_bs % 8 == 0 and a.ldout % 8 == 0 and a.out_bs % 8 == 0 and (not a.mask or (a.ldy % 8 == 0 and a.y_bs % 8 == 0)) and 16 // w.esz <= 8
    CH = 8 if kn["thin_ch"] == 8 and can8 else 4
    cblk = min(max(kn["thin_cblk"], 8 * CH), w.C, 256 * CH)
    sh = 0
    while (CH << sh) < cblk:
        sh += 1
    ppb = 256 >> sh
    M = w.N * w.H * w.W
    per = _ceil_div(M, kn["thin_blocks"] if kn["thin_blocks"] > 0 else 128)
    per = max(_ceil_div(per, 2 * ppb) * 2 * ppb, 8 * ppb)
    return CH, ppb, per, 0 if not a.mask else (1 if a.mask_is_x else 2)


def conv_bwd_pairs(a, w, kn):
    """Mirrors the pair condition of conv_bwd_dispatch: data-gradient and weight-gradient tiles in one launch"""
    if w is None or not (conv_is_vec(a) and wgrad_is_vec(w)):
        return False
    tx, ty, S = wgrad_plan(w, kn)
    nd = conv_blocks(a, 64, 64)
    return a.OC > 32 and not conv_takes_128(a) and nd <= kn["pair_max"] and nd + tx * ty * S <= 4096


def _conv_route(c, twin):
    kn = conv_knobs(c, twin)
    a, w = conv_problem(c, kn)
    scratch = a.esz == 2
    if a.mode == 1 and w is not None:
        if thin_bwd_ok(a, w) and not kn["no_thin_bwd"]:
            return "thin", thin_bwd_geometry(a, w, kn)[0], "thin"
        if conv_bwd_pairs(a, w, kn):
            return "pair", 1, "vec" if conv_epilogue_vec_ok(a) else "scalar"
    kind, n, _ = conv_plan(a, kn, scratch)
    return kind, n, "8p" if kind == "8p" else ("vec" if conv_epilogue_vec_ok(a) else "scalar")


_CONV_ROUTES = {}


def conv_route(c, twin=False):
    """(kind, n, epilogue copy) of the launch a single case makes: kind of CONV_TILE or "thin"; copy: vec (igemm_body's row-vectorised epilogue),
    scalar (its fallback), 8p (igemm8p_kernel's per-wave copy), thin"""
    key = (c[0], twin)
    if key not in _CONV_ROUTES:
        _CONV_ROUTES[key] = _conv_route(c, twin)
    return _CONV_ROUTES[key]


def conv_kind_name(route):
    kind, n, _ = route
    return "%s G%d" % (kind, n) if kind in ("64x64", "128x128") else kind


def conv_stat_n(c, twin=False):
    """fp32 additions in front of one fp64 atomic of the statistics, read from the kernels: igemm_body's row-vectorised epilogue adds BM / RP rows per
    thread and then RP partials per column; its scalar copy 16 TM rows per lane and the other half-wave; igemm8p_kernel 16 rows per lane, 8 row
    lanes by shuffles and the two wave rows: in each at most the tile's row count BM (64, 128 or 256).  thin_bwd_kernel: a thread's share of the
    block's pixels, then the block's pixel slots: at most the block's pixel count."""
    route = conv_route(c, twin)
    if route[0] == "thin":
        kn = conv_knobs(c, twin)
        a, w = conv_problem(c, kn)
        return min(thin_bwd_geometry(a, w, kn)[2], w.N * w.H * w.W)
    return CONV_TILE[route[0]][0]


def conv_gemm_dims(c):
    """(M, N) of the implicit GEMM whose epilogue the case runs: output pixels x output channels forward, input pixels x input channels backward"""
    f = conv_case_fields(c)
    if f.side == "fwd":
        return f.N * conv_out_size(f.H, f.k, f.stride, f.pad, f.dil) * conv_out_size(f.W, f.k, f.stride, f.pad, f.dil), f.OC
    return f.N * f.H * f.W, f.C


def conv_group_members(c):
    """the member cases of a grouped case (side multi: emrt_conv2d_dgrad_multi; side group: emrt_conv2d_group)"""
    return [conv_cases()[i] for i in c[14]]


def conv_group_is_one_launch(c):
    """Mirrors conv_group_launch: every problem on the vector path with OC > 32 and at most tile_cap 64x64 tiles, at most 4096 in all"""
    cap = 2048 if c[11] == "multi" else 4096
    ps = [conv_problem(m, dict(CONV_KNOBS))[0] for m in conv_group_members(c)]
    return all(conv_is_vec(a) and a.OC > 32 and conv_blocks(a, 64, 64) <= cap for a in ps) and sum(conv_blocks(a, 64, 64) for a in ps) <= 4096


def conv_in_domain(c):
    """the checks of emrt_conv2d (mode 0), emrt_conv2d_bwd, emrt_conv2d_dgrad_multi and emrt_conv2d_group, plus what the case format itself asks"""
    f = conv_case_fields(c)
    if f.side in ("multi", "group"):
        ms = conv_group_members(c)
        want = "bwd" if f.side == "multi" else "fwd"
        if len(ms) != 2 or any(m[11] != want or m[10] != f.dtype for m in ms) or ms[0][1:10] == ms[1][1:10]:
            return False
        if f.side == "group" and any(m[9] != 1 or "scale" in conv_feats(m) for m in ms):          # EmrtConvDesc: no dilation, no folded scale
            return False
        return (f.dtype != "f16" or f.side == "group") and all(conv_in_domain(m) for m in ms)
    if f.side not in ("fwd", "bwd") or f.dtype not in CONV_ESZ or f.inputs not in CONV_INPUTS:
        return False
    if not (f.N > 0 and f.H > 0 and f.W > 0 and f.C > 0 and f.OC > 0 and f.k > 0 and f.stride > 0 and f.pad >= 0 and f.dil >= 1):
        return False
    OH, OW = conv_out_size(f.H, f.k, f.stride, f.pad, f.dil), conv_out_size(f.W, f.k, f.stride, f.pad, f.dil)
    if OH <= 0 or OW <= 0:
        return False
    if f.side == "fwd" and (f.epilogue not in CONV_FWD_EPILOGUES or f.arm != "none"):
        return False
    if f.side == "bwd" and (f.epilogue not in CONV_BWD_EPILOGUES or f.arm not in CONV_ARMS or f.dtype == "f16"):
        return False
    if any(k not in CONV_KNOBS for k, _ in f.knobs + f.twin):
        return False
    try:
        t = conv_tensors(c)
    except (ValueError, KeyError):
        return False
    for v in t.values():          # strides at least the map; every view here keeps them multiples of 4 elements only by the tensor's own width
        if v.ld < v.ch + v.off or v.bs < v.pix * v.ld:
            return False
    feats = conv_feats(c)
    if "accumulate" in feats and "addend" in feats:
        return False
    if "stat_x" in feats and "mask" not in feats:
        return False
    if "mask" in feats and "out_f32" in feats:
        return False
    return max(v.bs * f.N for v in t.values()) <= MAX_ELEMS and f.OC * f.k * f.k * f.C <= MAX_ELEMS


_cv_L72k3 = (2, 9, 11, 72, 64, 3, 1, 1, 1)          # backward: M = 198 (four 64-row tiles, the last of 6 rows), 72 channels (two 64-column tiles), 9 k-tiles in bf16
_cv_L72k1 = (2, 9, 11, 72, 128, 1, 1, 0, 1)         # ... 2 k-tiles in bf16: fewer than the wave groups / copies asked for
_cv_L136k3 = (3, 10, 11, 136, 128, 3, 1, 1, 1)      # backward: M = 330 (three 128-row tiles, two 256-row tiles), 136 channels (two 128-column tiles)
_cv_L136k1 = (3, 10, 11, 136, 64, 1, 1, 0, 1)
_cv_L264k3 = (3, 10, 11, 264, 64, 3, 1, 1, 1)       # backward on the 256x256 kernel: two ragged M tiles, two ragged OC tiles, C = 64
_cv_L264k1 = (3, 10, 11, 264, 64, 1, 1, 0, 1)       # ... one k-tile: the loop's odd tail multiplies an all-zero tile
_cv_L24 = (3, 10, 11, 24, 64, 3, 1, 1, 1)           # backward of a layer with C <= 32: the ladder's 256x32 rung, vector epilogue
_cv_L6 = (3, 10, 11, 6, 64, 1, 1, 0, 1)             # ... scalar epilogue
_cv_L7 = (3, 10, 11, 7, 64, 3, 1, 1, 1)
_cv_L20 = (2, 9, 11, 20, 64, 3, 1, 1, 1)            # C % 8 != 0: the scalar epilogue by the channel count
_cv_L100 = (3, 10, 11, 100, 128, 3, 1, 1, 1)
_cv_F72k3 = (2, 9, 11, 64, 72, 3, 1, 1, 1)          # forward twins of the above
_cv_F72k1 = (2, 9, 11, 128, 72, 1, 1, 0, 1)
_cv_F136k3 = (3, 10, 11, 128, 136, 3, 1, 1, 1)
_cv_F136k1 = (3, 10, 11, 64, 136, 1, 1, 0, 1)
_cv_F264k3 = (3, 10, 11, 64, 264, 3, 1, 1, 1)
_cv_F264k1 = (3, 10, 11, 64, 264, 1, 1, 0, 1)
_cv_F24 = (3, 10, 11, 64, 24, 3, 1, 1, 1)
_cv_F6 = (3, 10, 11, 64, 6, 1, 1, 0, 1)
_cv_F7 = (3, 10, 11, 64, 7, 3, 1, 1, 1)
_cv_F20 = (2, 9, 11, 64, 20, 3, 1, 1, 1)
_cv_F100 = (3, 10, 11, 128, 100, 3, 1, 1, 1)
_cv_S3a = (1, 16, 16, 72, 64, 3, 2, 1, 1)           # stride 2: 256 input pixels = 4 parity classes of one 64-row tile each; 72 channels: a ragged column tile
_cv_S3b = (2, 8, 16, 64, 128, 3, 2, 1, 1)
_cv_S5a = (1, 16, 16, 72, 128, 5, 2, 2, 1)
_cv_S5b = (2, 8, 16, 64, 64, 5, 2, 2, 1)
_cv_S2a = (1, 16, 16, 72, 64, 2, 2, 0, 1)
_cv_S2b = (2, 8, 16, 64, 128, 2, 2, 0, 1)
_cv_T32o6 = (3, 10, 11, 32, 6, 1, 1, 0, 1)          # thin backward: 330 pixels = two pixel blocks of 256, the second ragged; C = 32: 4 channels per thread
_cv_T64o7 = (3, 10, 11, 64, 7, 1, 1, 0, 1)
_cv_T256o6 = (3, 10, 11, 256, 6, 1, 1, 0, 1)        # four channel chunks
_cv_T256o7 = (3, 10, 11, 256, 7, 1, 1, 0, 1)
_T = lambda t: (("conv_tile", t),)
_TP = lambda t: (("conv_tile", t), ("pair_max", 0))          # with dw the pair kernel would come first
_XK = lambda s: (("xk", s),)
_XKP = lambda s: (("xk", s), ("pair_max", 0))
_8P = lambda cm: (("conv_tile", 7), ("igemm8p_cmajor", cm))
_8PP = lambda cm: (("conv_tile", 7), ("igemm8p_cmajor", cm), ("pair_max", 0))
_S2TWIN = (("no_s2_dgrad", 1), ("conv_tile", 1), ("pair_max", 0))          # the generic 64x64 tile without a K split: the parity-class kernel's k order
_NOPAIR = (("pair_max", 0),)
_PAIR = (("pair_max", 1 << 30),)
_NOTHIN = (("no_thin_bwd", 1),)
_AMSX = "addend+mask+stats+stat_x"
_ACMS = "accumulate+mask+stats"
# (layer (N, H, W, C, OC, k, stride, pad, dilation), dtype, side, epilogue, backward arm, views, knobs, twin knobs, input recipe, what the row is there for)
_CONV_ROWS = (
    # ---- backward, 64x64 tile, one wave group ----
    (_cv_L72k3, "bf16", "bwd", _AMSX, "dx", "mask:ld8 addend:bs", _T(1), (), "ordinary", "64x64: every backward feature at once, ragged M and OC tiles"),
    (_cv_L72k3, "f32", "bwd", _AMSX, "dx+dw", "mask:ld2 dx:ld x:ld dy:bs", _TP(1), (), "ordinary", "64x64 fp32: a mask slice 8 bytes off the grid: the scalar epilogue by alignment alone"),
    (_cv_L72k1, "bf16", "bwd", _ACMS, "dx", "dx:ld+bs8 dy:ld", _T(1), (), "ordinary", "64x64: accumulate into a padded slice of dx"),
    (_cv_L20, "bf16", "bwd", "accumulate", "dx+dw+dbias", "x:ld+bs", _TP(1), (), "ordinary", "64x64: 20 channels, the scalar epilogue by the channel count"),
    (_cv_L72k3, "bf16", "bwd", "none", "dx", "", _T(1), (), "corner", "64x64: corner pixels only, exact zeros elsewhere"),
    (_cv_L72k3, "bf16", "bwd", "mask", "dx", "mask:bs", _T(1), (), "lastpixel", "64x64: dy at the last pixel, masked"),
    # ---- two and four wave groups ----
    (_cv_L72k3, "bf16", "bwd", _AMSX, "dx", "statx:ld16 addend:ld+bs", _T(5), (), "ordinary", "64x64 G2: the summed accumulators under every feature"),
    (_cv_L72k3, "bf16", "bwd", _AMSX, "dx", "addend:ld4", _T(5), (), "ordinary", "64x64 G2: an addend slice 8 bytes off the grid: scalar epilogue"),
    (_cv_L72k1, "f32", "bwd", _ACMS, "dx+dw", "dy:bs x:bs", _TP(5), (), "ordinary", "64x64 G2 fp32, 4 k-tiles on two groups"),
    (_cv_L72k3, "f32", "bwd", "accumulate", "dx", "dx:ld2", _T(5), (), "ordinary", "64x64 G2: dx itself off the grid: scalar epilogue, accumulate"),
    (_cv_L72k3, "bf16", "bwd", _AMSX, "dx", "mask:ld+bs statx:bs", _T(6), (), "ordinary", "64x64 G4"),
    (_cv_L72k1, "bf16", "bwd", _AMSX, "dx+dw", "statx:ld4 x:ld+bs dy:ld", _TP(6), (), "ordinary", "64x64 G4: 2 k-tiles on four groups (two walk nothing); stat_x off the grid: scalar"),
    (_cv_L72k3, "f32", "bwd", _ACMS, "dx", "", _T(6), (), "ordinary", "64x64 G4 fp32"),
    (_cv_L20, "f32", "bwd", "accumulate+stats", "dx", "dx:bs", _T(6), (), "ordinary", "64x64 G4: 20 channels, scalar epilogue with statistics"),
    # ---- 128x64 ----
    (_cv_L72k3, "bf16", "bwd", _AMSX, "dx", "dx:ld8", _T(2), (), "ordinary", "128x64: 198 rows = two tiles, the second of 70 rows"),
    (_cv_L72k3, "f32", "bwd", _AMSX, "dx+dw+dbias", "mask:ld+bs2 x:bs dy:ld+bs", _TP(2), (), "ordinary", "128x64 fp32, scalar epilogue by a mask slice off the grid"),
    (_cv_L72k1, "bf16", "bwd", _ACMS, "dx", "mask:ld", _T(2), (), "ordinary", "128x64: accumulate"),
    (_cv_L20, "bf16", "bwd", "accumulate", "dx", "", _T(2), (), "ordinary", "128x64: 20 channels, scalar epilogue"),
    # ---- 128x128, one and two wave groups ----
    (_cv_L136k3, "bf16", "bwd", _AMSX, "dx", "mask:bs addend:ld8", _T(3), (), "ordinary", "128x128: 330 rows = three tiles, 136 channels = two tiles"),
    (_cv_L100, "bf16", "bwd", _AMSX, "dx", "", _T(3), (), "ordinary", "128x128: 100 channels, scalar epilogue"),
    (_cv_L136k1, "f32", "bwd", _ACMS, "dx+dw", "x:ld8 dy:ld", _TP(3), (), "ordinary", "128x128 fp32, accumulate"),
    (_cv_L136k3, "f32", "bwd", "accumulate", "dx", "dx:ld+bs2", _T(3), (), "ordinary", "128x128 fp32: dx off the grid, scalar epilogue"),
    (_cv_L136k3, "bf16", "bwd", _AMSX, "dx", "statx:ld+bs8", _T(8), (), "ordinary", "128x128 G2: K split over two wave groups"),
    (_cv_L136k1, "bf16", "bwd", _AMSX, "dx+dw", "mask:ld4", _TP(8), (), "ordinary", "128x128 G2: one k-tile on two groups; scalar epilogue by alignment"),
    (_cv_L136k3, "bf16", "bwd", _ACMS, "dx", "dy:ld+bs", _T(8), (), "ordinary", "128x128 G2: accumulate"),
    (_cv_L100, "bf16", "bwd", "accumulate+stats", "dx", "", _T(8), (), "ordinary", "128x128 G2: 100 channels, scalar epilogue, accumulate with statistics"),
    # ---- 256x32: the ladder's rung for a layer with C <= 32, and forced ----
    (_cv_L24, "bf16", "bwd", "mask+stats", "dx+dw", "mask:ld8", (), (), "ordinary", "256x32 by the ladder: 24 channels take the vector epilogue"),
    (_cv_L6, "bf16", "bwd", "mask+stats", "dx+dw+dbias", "", (), (), "ordinary", "256x32: 6 channels, scalar epilogue, mask + statistics"),
    (_cv_L7, "f32", "bwd", "mask+stats", "dx", "mask:bs", (), (), "ordinary", "256x32: 7 channels"),
    (_cv_L24, "f32", "bwd", _AMSX, "dx", "addend:ld4", (), (), "ordinary", "256x32 fp32: vector epilogue with every feature"),
    (_cv_L7, "bf16", "bwd", _AMSX, "dx", "", (), (), "ordinary", "256x32: 7 channels with every feature"),
    (_cv_L24, "bf16", "bwd", _ACMS, "dx", "dx:ld+bs8", (), (), "ordinary", "256x32: accumulate into a slice"),
    (_cv_L6, "f32", "bwd", "accumulate", "dx", "", (), (), "ordinary", "256x32: accumulate, scalar"),
    (_cv_L72k3, "bf16", "bwd", _AMSX, "dx", "", _T(4), (), "ordinary", "256x32 forced on 72 channels: three column tiles, the last of 8"),
    # ---- cross-block K split ----
    (_cv_L72k3, "bf16", "bwd", _AMSX, "dx", "mask:ld8", _XK(2), (), "ordinary", "xk = 2: 9 k-tiles as 5 + 4"),
    (_cv_L72k3, "bf16", "bwd", "mask+stats+stat_x", "dx+dw", "statx:ld+bs", _XKP(3), (), "ordinary", "xk = 3: three copies of 3 k-tiles"),
    (_cv_L72k3, "bf16", "bwd", "addend", "dx", "addend:ld+bs16 dx:ld", _XK(8), (), "ordinary", "xk = 8: cut down to 5 copies of 2 k-tiles, the last of one"),
    (_cv_L72k1, "bf16", "bwd", _ACMS, "dx", "", _XK(8), (), "ordinary", "xk = 8 on 2 k-tiles: fewer k-tiles than copies asked for"),
    (_cv_L72k3, "bf16", "bwd", "accumulate", "dx", "dx:bs", _XK(2), (), "ordinary", "xk = 2: accumulate"),
    (_cv_L72k1, "bf16", "bwd", _AMSX, "dx", "", _XK(3), (), "ordinary", "xk = 3 on 2 k-tiles"),
    # ---- parity-class kernel, each with its generic twin (bit-identical dx) ----
    (_cv_S3a, "bf16", "bwd", _AMSX, "dx", "dx:ld+bs8 mask:ld8", (), _S2TWIN, "ordinary", "s2 3x3: the remapped row finds mask, stat_x and addend; strided dx"),
    (_cv_S3b, "bf16", "bwd", "mask+stats+stat_x", "dx+dw", "mask:bs statx:ld", _NOPAIR, _S2TWIN, "ordinary", "s2 3x3 on 2 x 8 x 16: a class spans both images"),
    (_cv_S5a, "bf16", "bwd", "mask+scale", "dx", "mask:ld+bs", (), _S2TWIN, "ordinary", "s2 5x5 pad 2: mask_scale on the parity-class path"),
    (_cv_S5b, "f32", "bwd", _ACMS, "dx", "dx:ld4", (), _S2TWIN, "ordinary", "s2 5x5 fp32: accumulate into a strided dx"),
    (_cv_S2a, "bf16", "bwd", "addend", "dx", "addend:ld8", (), _S2TWIN, "ordinary", "s2 2x2 pad 0: one tap per class"),
    (_cv_S2b, "f32", "bwd", "accumulate", "dx", "", (), _S2TWIN, "ordinary", "s2 2x2 fp32"),
    (_cv_S3a, "f32", "bwd", "stats", "dx", "", (), _S2TWIN, "ordinary", "s2 3x3 fp32: statistics alone"),
    (_cv_S3b, "bf16", "bwd", _AMSX, "dx", "statx:ld+bs8 addend:bs", (), _S2TWIN, "lastpixel", "s2: dy at the last pixel, every feature"),
    # ---- pair kernel ----
    (_cv_L72k3, "bf16", "bwd", "mask+stats", "dx+dw+dbias", "mask:ld8", _PAIR, (), "ordinary", "pair: mask + statistics on the data-gradient half, dw from random contents"),
    (_cv_L72k3, "f32", "bwd", "mask+stats", "dx+dw+dbias", "", _PAIR, (), "ordinary", "pair fp32"),
    (_cv_L72k1, "bf16", "bwd", _AMSX, "dx+dw", "addend:ld+bs dx:bs", _PAIR, (), "ordinary", "pair: every feature"),
    (_cv_L136k1, "f32", "bwd", _AMSX, "dx+dw+dbias", "", _PAIR, (), "ordinary", "pair fp32, 330 rows"),
    (_cv_L72k3, "bf16", "bwd", _ACMS, "dx+dw", "", _PAIR, (), "ordinary", "pair: accumulate"),
    (_cv_L72k3, "f32", "bwd", "accumulate", "dx+dw+dbias", "dx:ld4", _PAIR, (), "corner", "pair fp32: accumulate, corner pixels"),
    # ---- 256x256 LDS-DMA kernel: k = 3 and k = 1, both k orders, every backward epilogue ----
    (_cv_L264k3, "bf16", "bwd", "none", "dx", "", _8P(0), (), "ordinary", "8p 3x3 tap-major: plain"),
    (_cv_L264k3, "bf16", "bwd", "mask+stats+stat_x", "dx", "mask:ld8 statx:bs", _8P(0), (), "ordinary", "8p: strided mask, stat_x"),
    (_cv_L264k3, "bf16", "bwd", _AMSX, "dx+dw", "mask:ld+bs8 addend:ld16", _8PP(0), (), "ordinary", "8p: strided mask and addend that keep it eligible"),
    (_cv_L264k3, "bf16", "bwd", "accumulate", "dx", "dx:ld8", _8P(0), (), "ordinary", "8p: accumulate into a slice"),
    (_cv_L264k3, "bf16", "bwd", "stats", "dx", "", _8P(1), (), "ordinary", "8p 3x3 channel-block-major: statistics"),
    (_cv_L264k3, "bf16", "bwd", "mask", "dx", "mask:bs", _8P(1), (), "corner", "8p cmajor: mask, corner pixels"),
    (_cv_L264k3, "bf16", "bwd", "addend", "dx", "addend:ld+bs", _8P(1), (), "ordinary", "8p cmajor: addend"),
    (_cv_L264k3, "bf16", "bwd", _ACMS, "dx+dw+dbias", "", _8PP(1), (), "ordinary", "8p cmajor: accumulate + mask + statistics"),
    (_cv_L264k1, "bf16", "bwd", "mask+stats", "dx", "mask:ld", _8P(0), (), "ordinary", "8p 1x1: one k-tile"),
    (_cv_L264k1, "bf16", "bwd", "mask+scale", "dx", "", _8P(0), (), "ordinary", "8p 1x1: mask_scale"),
    (_cv_L264k1, "bf16", "bwd", _AMSX, "dx", "mask:ld+bs statx:ld8 addend:bs", _8P(0), (), "ordinary", "8p 1x1: every operand strided"),
    (_cv_L264k1, "bf16", "bwd", "mask+stats+stat_x", "dx", "statx:ld+bs", _8P(1), (), "ordinary", "8p 1x1 cmajor"),
    (_cv_L264k1, "bf16", "bwd", _ACMS, "dx", "dx:ld+bs", _8P(1), (), "lastpixel", "8p 1x1 cmajor: accumulate, dy at the last pixel"),
    (_cv_L264k3, "bf16", "bwd", _AMSX, "dx", "mask:ld4", _8P(0), (), "ordinary", "8p refused: a mask slice off the grid sends conv_tile = 7 down the ladder to the 64x64 tile, scalar epilogue"),
    # ---- thin backward, each with the generic kernels as twin ----
    (_cv_T32o6, "bf16", "bwd", "none", "dx+dw+dbias", "", (), _NOTHIN, "ordinary", "thin MASK 0, C = 32: 4 channels per thread"),
    (_cv_T64o7, "f32", "bwd", "stats", "dx+dw", "x:ld", (), _NOTHIN, "ordinary", "thin MASK 0 with statistics, 7 output channels"),
    (_cv_T256o6, "bf16", "bwd", "accumulate", "dx+dw+dbias", "dx:ld+bs8", (), _NOTHIN, "ordinary", "thin ACC: four channel chunks"),
    (_cv_T64o7, "bf16", "bwd", "accumulate+stats", "dx+dw", "", (), _NOTHIN, "ordinary", "thin ACC with statistics"),
    (_cv_T64o7, "bf16", "bwd", "maskx", "dx+dw+dbias", "x:bs", (), _NOTHIN, "ordinary", "thin MASK 1: mask_y is x"),
    (_cv_T256o7, "f32", "bwd", "maskx+stats", "dx+dw", "", (), _NOTHIN, "ordinary", "thin MASK 1 with statistics, fp32"),
    (_cv_T32o6, "f32", "bwd", "mask", "dx+dw", "mask:ld4", (), _NOTHIN, "ordinary", "thin MASK 2, C = 32 fp32"),
    (_cv_T256o6, "bf16", "bwd", "mask+stats", "dx+dw+dbias", "mask:ld+bs8", (), _NOTHIN, "ordinary", "thin MASK 2 with statistics"),
    (_cv_T64o7, "bf16", "bwd", "mask+scale", "dx+dw", "mask:bs", (), _NOTHIN, "lastpixel", "thin MASK 2 with mask_scale, dy at the last pixel"),
    (_cv_T256o6, "bf16", "bwd", _ACMS, "dx+dw", "", (), (), "ordinary", "accumulate + mask at a thin shape: refused by thin_bwd_ok, the generic kernels"),
    # ---- forward ----
    (_cv_F72k3, "bf16", "fwd", "bias+residual+relu", "none", "res:ld8 out:bs", _T(1), (), "ordinary", "64x64 forward: the bottleneck's join"),
    (_cv_F20, "f32", "fwd", "fold+relu", "none", "in:ld", _T(1), (), "ordinary", "64x64: 20 output channels, scalar epilogue, folded BatchNorm with negative scales"),
    (_cv_F100, "bf16", "fwd", "bias+residual+relu", "none", "res:bs", _T(1), (), "ordinary", "64x64: 100 output channels, scalar epilogue"),
    (_cv_F72k3, "bf16", "fwd", "none", "none", "in:ld+bs8", _T(1), (), "corner", "64x64 forward, corner pixels"),
    (_cv_F72k3, "bf16", "fwd", "stats+relu", "none", "out:ld8", _T(5), (), "ordinary", "64x64 G2 forward: statistics of the stored output"),
    (_cv_F72k1, "f32", "fwd", "residual", "none", "res:ld2", _T(5), (), "ordinary", "64x64 G2 fp32: residual slice off the grid, scalar epilogue"),
    (_cv_F72k1, "bf16", "fwd", "fold+relu", "none", "in:bs", _T(6), (), "ordinary", "64x64 G4 forward"),
    (_cv_F72k3, "bf16", "fwd", "stats", "none", "out:ld4", _T(6), (), "ordinary", "64x64 G4: output slice off the grid, scalar epilogue with statistics"),
    (_cv_F72k3, "bf16", "fwd", "out_f32+bias", "none", "out:ld4", _T(2), (), "ordinary", "128x64: fp32 output slice 16 bytes into its buffer: vector epilogue"),
    (_cv_F20, "bf16", "fwd", "fold", "none", "", _T(2), (), "ordinary", "128x64: 20 output channels, scalar epilogue"),
    (_cv_F72k3, "f32", "fwd", "relu", "none", "in:ld+bs", _T(2), (), "ordinary", "128x64 fp32"),
    (_cv_F136k3, "bf16", "fwd", "bias+residual+relu", "none", "res:ld+bs8", _T(3), (), "ordinary", "128x128 forward"),
    (_cv_F100, "f32", "fwd", "stats+relu", "none", "", _T(3), (), "ordinary", "128x128 fp32: 100 output channels, scalar epilogue with statistics"),
    (_cv_F136k1, "f32", "fwd", "bias", "none", "out:ld+bs", _T(3), (), "lastpixel", "128x128 fp32 1x1, x at the last pixel"),
    (_cv_F136k3, "bf16", "fwd", "fold", "none", "out:bs", _T(8), (), "ordinary", "128x128 G2 forward"),
    (_cv_F136k1, "bf16", "fwd", "out_f32", "none", "out:ld2", _T(8), (), "ordinary", "128x128 G2: fp32 output 8 bytes off the grid, scalar epilogue"),
    (_cv_F24, "bf16", "fwd", "stats+relu", "none", "out:ld8", (), (), "ordinary", "256x32 forward by the ladder, vector epilogue"),
    (_cv_F6, "bf16", "fwd", "bias", "none", "", (), (), "ordinary", "256x32: 6 output channels"),
    (_cv_F7, "f32", "fwd", "out_f32+bias", "none", "in:ld", (), (), "ordinary", "256x32 fp32: 7 output channels"),
    (_cv_F24, "f32", "fwd", "relu", "none", "", (), (), "ordinary", "256x32 fp32"),
    (_cv_F72k3, "bf16", "fwd", "bias+residual+relu", "none", "res:ld+bs out:ld", _XK(2), (), "ordinary", "xk = 2 forward"),
    (_cv_F72k3, "bf16", "fwd", "stats+relu", "none", "", _XK(3), (), "ordinary", "xk = 3 forward with statistics"),
    (_cv_F72k1, "bf16", "fwd", "fold+relu", "none", "out:bs", _XK(8), (), "ordinary", "xk = 8 on 4 k-tiles"),
    (_cv_F264k3, "bf16", "fwd", "out_f32", "none", "", _8P(0), (), "ordinary", "8p forward: fp32 output"),
    (_cv_F264k3, "bf16", "fwd", "bias+residual+relu", "none", "res:ld8 out:ld+bs", _8P(0), (), "ordinary", "8p forward: join"),
    (_cv_F264k3, "bf16", "fwd", "fold+relu", "none", "in:ld+bs", _8P(1), (), "ordinary", "8p forward cmajor"),
    (_cv_F264k1, "bf16", "fwd", "stats+relu", "none", "", _8P(1), (), "ordinary", "8p forward 1x1 with statistics"),
    (_cv_F264k1, "bf16", "fwd", "out_f32+bias", "none", "out:ld4", _8P(0), (), "ordinary", "8p forward: fp32 output slice"),
    (_cv_F264k1, "bf16", "fwd", "fold", "none", "", _8P(0), (), "lastpixel", "8p forward: folded BatchNorm, x at the last pixel"),
    (_cv_F264k3, "bf16", "fwd", "residual", "none", "res:bs", _8P(0), (), "ordinary", "8p forward: residual"),
    (_cv_F264k1, "bf16", "fwd", "stats", "none", "out:ld+bs8", _8P(0), (), "ordinary", "8p forward: statistics"),
    (_cv_F264k3, "bf16", "fwd", "relu", "none", "", _8P(0), (), "ordinary", "8p forward: ReLU alone"),
    (_cv_F72k3, "bf16", "fwd", "bias", "none", "", (), (), "ordinary", "the dispatcher's own choice, bias"),
    (_cv_F136k3, "f32", "fwd", "none", "none", "", (), (), "ordinary", "the dispatcher's own choice, fp32"),
    (_cv_F136k1, "bf16", "fwd", "residual", "none", "", (), (), "ordinary", "the dispatcher's own choice, residual"),
    # ---- forward-only float16 ----
    (_cv_F72k3, "f16", "fwd", "fold", "none", "out:ld8", _T(1), (), "ordinary", "fp16 64x64: folded BatchNorm"),
    (_cv_F264k3, "f16", "fwd", "bias+residual+relu", "none", "res:ld", _8P(0), (), "ordinary", "fp16 on the 256x256 kernel"),
    (_cv_F136k3, "f16", "fwd", "relu", "none", "", _T(3), (), "ordinary", "fp16 128x128"),
    (_cv_F72k1, "f16", "fwd", "bias", "none", "in:bs", _XK(2), (), "ordinary", "fp16 cross-block split"),
    (_cv_F6, "f16", "fwd", "out_f32", "none", "", (), (), "ordinary", "fp16 256x32, fp32 output, scalar epilogue"),
    (_cv_F20, "f16", "fwd", "out_f32+bias", "none", "", _T(1), (), "ordinary", "fp16 64x64: fp32 output of 20 channels, scalar epilogue"),
    # ---- what the lists above left with one case ----
    (_cv_F136k1, "bf16", "fwd", "out_f32", "none", "", _T(3), (), "ordinary", "128x128: fp32 output through the vector epilogue"),
    (_cv_L72k1, "bf16", "bwd", "mask+scale", "dx", "", _T(2), (), "ordinary", "128x64: mask_scale, vector epilogue"),
    (_cv_L20, "bf16", "bwd", "mask+scale", "dx", "", _T(1), (), "ordinary", "64x64: mask_scale, scalar epilogue"),
    (_cv_L100, "f32", "bwd", "mask+scale", "dx", "mask:bs", _T(3), (), "ordinary", "128x128 fp32: mask_scale, scalar epilogue"),
    (_cv_T32o6, "bf16", "bwd", "maskx+stats", "dx+dw+dbias", "", (), _NOTHIN, "ordinary", "thin MASK 1 with statistics at C = 32"),
    (_cv_T256o7, "bf16", "bwd", "maskx", "dx+dw", "x:ld8", (), _NOTHIN, "ordinary", "thin MASK 1 on a slice of a wider x"),
)
# two unequal problems of the list in one launch: (entry point, (row, row), dtype, what it is there for)
_CONV_GROUP_ROWS = (
    ("multi", (0, 2), "bf16", "dgrad_multi: every feature beside accumulate + mask + statistics"),
    ("multi", (36, 39), "bf16", "dgrad_multi: two of the xk cases' problems side by side on the grouped 64x64 kernel"),
    ("multi", (1, 8), "f32", "dgrad_multi fp32: a scalar-epilogue problem beside a vector one"),
    ("group", (80, 82), "bf16", "conv2d_group: a scalar-epilogue join beside statistics"),
    ("group", (83, 91), "f32", "conv2d_group fp32: a 1x1 residual off the grid beside a 330-pixel 1x1"),
    ("group", (115, 116), "f16", "conv2d_group fp16"),
)


def conv_cases(seed=2212):
    """(id, N, H, W, C, OC, k, stride, pad, dilation, dtype, side, epilogue, arm, views, knobs, twin, inputs, why, seed); a grouped case has side
    multi / group, zeros for the layer and the indices of its two member cases in the views field"""
    if seed not in _CONV_CASES:
        out = [("conv%d-%d" % (seed, i),) + row[0] + row[1:] + (seed + i,) for i, row in enumerate(_CONV_ROWS)]
        for side, members, dtype, why in _CONV_GROUP_ROWS:
            out.append(("conv%d-%d" % (seed, len(out)),) + (0,) * 9 + (dtype, side, "none", "none", members, (), (), "ordinary", why, seed + len(out)))
        _CONV_CASES[seed] = out
    return _CONV_CASES[seed]


_CONV_CASES = {}


def _cv_single(c):
    return c[11] in ("fwd", "bwd")


def _cv_kind(c):
    return conv_kind_name(conv_route(c)) if _cv_single(c) else None


def _cv_copy(c):
    return conv_route(c)[2] if _cv_single(c) else None


def _cv_has(c, feat):
    return _cv_single(c) and feat in conv_feats(c)


def _cv_ragged(c, axis):
    if not _cv_single(c) or conv_route(c)[0] == "thin":
        return False
    bm, bn = CONV_TILE[conv_route(c)[0]]
    return conv_gemm_dims(c)[axis] % (bm, bn)[axis] != 0


def _cv_view_kind(c, role):
    if not _cv_single(c) or role not in CONV_ROLES[c[11]]:
        return None
    t = conv_tensors(c)
    return t[role].kind if role in t and not (role == "mask" and "mask_is_x" in conv_feats(c)) else None


def _cv_off_grid_only(c):
    """the scalar epilogue for alignment alone: channel count a multiple of 8, some epilogue operand's slice off the 16-byte grid"""
    return _cv_copy(c) == "scalar" and conv_gemm_dims(c)[1] % 8 == 0


_CV_COPIES = {"64x64 G1": ("vec", "scalar"), "64x64 G2": ("vec", "scalar"), "64x64 G4": ("vec", "scalar"), "128x64": ("vec", "scalar"),
              "128x128 G1": ("vec", "scalar"), "128x128 G2": ("vec", "scalar"), "256x32": ("vec", "scalar"), "xk": ("vec",), "s2": ("vec",), "8p": ("8p",),
              "pair": ("vec",), "thin": ("thin",)}
_CV_BWD_FEATS = ("mask", "stats", "stat_x", "addend", "accumulate")
_CV_FWD_FEATS = ("bias", "scale", "residual", "relu", "stats", "out_f32")
_CV_FWD_KINDS = ("64x64 G1", "64x64 G2", "64x64 G4", "128x64", "128x128 G1", "128x128 G2", "256x32", "xk", "8p")


def _cv_l(fn, *args):
    return lambda c: fn(c, *args)


CONV_REGIMES = [("%s, %s epilogue" % (k, cp), _cv_l(lambda c, k_, cp_: _cv_kind(c) == k_ and _cv_copy(c) == cp_, k, cp)) for k in CONV_KINDS for cp in _CV_COPIES[k]] + [
    ("%s: backward with %s" % (k, ft), _cv_l(lambda c, k_, ft_: c[11] == "bwd" and _cv_kind(c) == k_ and _cv_has(c, ft_), k, ft))
    for k in CONV_KINDS for ft in _CV_BWD_FEATS if not (k == "thin" and ft in ("stat_x", "addend"))] + [
    ("%s: forward" % k, _cv_l(lambda c, k_: c[11] == "fwd" and _cv_kind(c) == k_, k)) for k in _CV_FWD_KINDS] + [
    ("%s epilogue, forward with %s" % (cp, ft), _cv_l(lambda c, cp_, ft_: c[11] == "fwd" and _cv_copy(c) == cp_ and _cv_has(c, ft_), cp, ft))
    for cp in ("vec", "scalar", "8p") for ft in _CV_FWD_FEATS] + [
    ("%s epilogue, backward with %s" % (cp, ft), _cv_l(lambda c, cp_, ft_: c[11] == "bwd" and _cv_copy(c) == cp_ and _cv_has(c, ft_), cp, ft))
    for cp in ("vec", "scalar") for ft in _CV_BWD_FEATS + ("mask_scale",)] + [
    ("%s: ragged last M tile" % k, _cv_l(lambda c, k_: _cv_kind(c) == k_ and _cv_ragged(c, 0), k)) for k in CONV_KINDS if k not in ("s2", "thin")] + [
    ("%s: ragged last OC tile" % k, _cv_l(lambda c, k_: _cv_kind(c) == k_ and _cv_ragged(c, 1), k)) for k in CONV_KINDS if k != "thin"] + [
    ("scalar epilogue by alignment alone, %s" % side, _cv_l(lambda c, s_: c[11] == s_ and _cv_off_grid_only(c), side)) for side in ("fwd", "bwd")] + [
    ("%s view: %s" % (role, v), _cv_l(lambda c, r_, v_: _cv_view_kind(c, r_) == v_, role, v)) for side in ("fwd", "bwd") for role in CONV_ROLES[side] for v in CONV_VIEWS] + [
    ("%s, %s" % (side, d), _cv_l(lambda c, s_, d_: c[11] == s_ and c[10] == d_, side, d)) for side, d in (("fwd", "f32"), ("fwd", "bf16"), ("fwd", "f16"), ("bwd", "f32"), ("bwd", "bf16"))] + [
    ("forward epilogue: %s" % e, _cv_l(lambda c, e_: c[11] == "fwd" and c[12] == e_, e)) for e in CONV_FWD_EPILOGUES] + [
    ("backward epilogue: %s" % e, _cv_l(lambda c, e_: c[11] == "bwd" and c[12] == e_, e)) for e in CONV_BWD_EPILOGUES] + [
    ("backward arm: %s" % arm, _cv_l(lambda c, a_: c[11] == "bwd" and c[13] == a_, arm)) for arm in CONV_ARMS] + [
    ("xk = %d asked" % s, _cv_l(lambda c, s_: _cv_kind(c) == "xk" and dict(c[15]).get("xk") == s_, s)) for s in (2, 3, 8)] + [
    ("xk: fewer k-tiles than the copies asked for", lambda c: _cv_kind(c) == "xk" and conv_k_tiles(conv_problem(c)[0]) < dict(c[15]).get("xk", 0)),
    ("8p: k = 3, tap-major", lambda c: _cv_kind(c) == "8p" and c[6] == 3 and not dict(c[15]).get("igemm8p_cmajor")),
    ("8p: k = 3, channel-block-major", lambda c: _cv_kind(c) == "8p" and c[6] == 3 and dict(c[15]).get("igemm8p_cmajor") == 1),
    ("8p: k = 1, tap-major", lambda c: _cv_kind(c) == "8p" and c[6] == 1 and not dict(c[15]).get("igemm8p_cmajor")),
    ("8p: k = 1, channel-block-major", lambda c: _cv_kind(c) == "8p" and c[6] == 1 and dict(c[15]).get("igemm8p_cmajor") == 1),
    ("8p asked, refused by igemm8p_ok: the ladder's kernel", lambda c: _cv_single(c) and dict(c[15]).get("conv_tile") == 7 and _cv_kind(c) != "8p"),
    ("s2: k = 3 pad 1", lambda c: _cv_kind(c) == "s2" and (c[6], c[8]) == (3, 1)),
    ("s2: k = 5 pad 2", lambda c: _cv_kind(c) == "s2" and (c[6], c[8]) == (5, 2)),
    ("s2: k = 2 pad 0", lambda c: _cv_kind(c) == "s2" and (c[6], c[8]) == (2, 0)),
    ("s2: 1 x 16 x 16", lambda c: _cv_kind(c) == "s2" and c[1:4] == (1, 16, 16)),
    ("s2: 2 x 8 x 16", lambda c: _cv_kind(c) == "s2" and c[1:4] == (2, 8, 16)),
    ("s2: generic twin, bit-identical dx", lambda c: _cv_kind(c) == "s2" and conv_route(c, True)[:2] == ("64x64", 1)),
    ("thin: MASK 0", lambda c: _cv_kind(c) == "thin" and not _cv_has(c, "mask")),
    ("thin: MASK 1 (mask_y is x)", lambda c: _cv_kind(c) == "thin" and _cv_has(c, "mask_is_x")),
    ("thin: MASK 2", lambda c: _cv_kind(c) == "thin" and _cv_has(c, "mask") and not _cv_has(c, "mask_is_x")),
    ("thin: 4 channels per thread", lambda c: _cv_kind(c) == "thin" and conv_route(c)[1] == 4),
    ("thin: 8 channels per thread", lambda c: _cv_kind(c) == "thin" and conv_route(c)[1] == 8),
    ("thin: generic twin", lambda c: _cv_kind(c) == "thin" and conv_route(c, True)[0] != "thin"),
    ("thin shape refused by thin_bwd_ok", lambda c: _cv_single(c) and c[11] == "bwd" and c[6] == 1 and c[5] <= 8 and "dw" in c[13] and _cv_kind(c) != "thin"),
    ("grouped launch: emrt_conv2d_dgrad_multi", lambda c: c[11] == "multi" and conv_group_is_one_launch(c)),
    ("grouped launch: emrt_conv2d_group", lambda c: c[11] == "group" and conv_group_is_one_launch(c)),
] + [("inputs: %s" % r, _cv_l(lambda c, r_: _cv_single(c) and c[17] == r_, r)) for r in CONV_INPUTS]


# ---------------------------------------------------------------------------------------------------------------------------------
# the losses: emrt_softmax_ce_* / emrt_wce_* / emrt_ohem_ce_* (csrc/loss.hip), emrt_lx_dice_ce_* (csrc/loss_ext/loss_ext.hip), all on the pixel
# core of csrc/loss_pixel.hpp (tests/test_gpu_loss_fuzz.py; inputs and float64 references: tests/loss_step_reference.py).  Written out like
# the gconv list.  The host arithmetic below carries the names the C++ has.
# ---------------------------------------------------------------------------------------------------------------------------------
LOSS_LONG_MAX_ELEMS = 2 * 1025 * 1024          # logits of one head, for the four cases that send a backward kernel round its loop twice
LOSS_FAMILIES = ("ce", "wce", "ohem", "dice")
LOSS_FORMS = ("single", "pair")
LOSS_LABELS = ("none", "tenth", "all", "allbut1", "oneclass")          # which pixels carry the ignore index (oneclass: a tenth, the rest one class)
LOSS_LOGITS = ("ordinary", "confident", "shift+", "shift-", "wide", "constant", "grid")
LOSS_CW = ("none", "random", "onezero", "zeropresent")
LOSS_FWD_BLOCKS, LOSS_BWD_BLOCKS, LOSS_HIST_BLOCKS = 1024, 4096, 128          # wce_forward / ohem_forward: loss.hip:359,388; wce_backward / ohem_backward: 372,406; OH_HIST_BLOCKS: 25,391
LX_MAX_BLOCKS, LX_BWD_BLOCKS, LX_CHUNK, LX_HEAD, LX_MAX_CLASSES = 1024, 4096, 8, 3, 64          # loss_ext.hip:41-44, EMRT_LX_MAX_CLASSES


def stream_grid(npix, cap):
    """grid of a streaming launch: one thread per pixel, capped.  loss_pixel.hpp:56-59"""
    g = (npix + 255) // 256
    return cap if g > cap else 1 if g < 1 else g


def shape_ok(N, C, H, W):
    """loss_pixel.hpp:61"""
    return N >= 1 and C >= 1 and H >= 1 and W >= 1 and N * H * W < (1 << 31)


def lx_chunks(C):
    """loss_ext.hip:48"""
    return (C + LX_CHUNK - 1) // LX_CHUNK


def lx_stride(C):
    """floats per block of the Dice forward's workspace.  loss_ext.hip:49"""
    return LX_HEAD + lx_chunks(C) * 3 * LX_CHUNK


def loss_npix(c):
    return c[3] * c[5] * c[6]


def loss_grids(c):
    """(forward grid, backward grid, histogram grid or None) of a case's family: wce_forward / wce_backward / ohem_forward / ohem_backward
    (loss.hip:359,372,388,391,406), dice_forward / dice_backward (loss_ext.hip:296,313)"""
    n = loss_npix(c)
    if c[1] == "dice":
        return stream_grid(n, LX_MAX_BLOCKS), stream_grid(n, LX_BWD_BLOCKS), None
    return stream_grid(n, LOSS_FWD_BLOCKS), stream_grid(n, LOSS_BWD_BLOCKS), (stream_grid(n, LOSS_HIST_BLOCKS) if c[1] == "ohem" else None)


def loss_depth(npix, grid):
    """pixels one thread of a grid-stride loop takes at most: the fp32 additions in front of the block's reduction"""
    return _ceil_div(npix, grid * 256)


def loss_in_domain(c):
    """the EMRT_REQUIRE / LX_REQUIRE lines of the entry points; a label pattern outside LOSS_LABELS (a label outside [0, C) that is not the
    ignore index: include/emrt_hip_loss.h puts it outside the contract) is refused here"""
    _, fam, form, N, C, H, W, ign, labels, logits, cw, hw, up, thresh, min_kept, dice, _, _ = c
    if fam not in LOSS_FAMILIES or form not in LOSS_FORMS or labels not in LOSS_LABELS or logits not in LOSS_LOGITS or cw not in LOSS_CW:
        return False
    if not shape_ok(N, C, H, W) or len(hw) != 2:
        return False
    if 0 <= ign < C and labels == "none":          # the ignored class's own pixels are ignored: "none ignored" cannot be drawn
        return False
    if fam in ("ce", "ohem") and cw != "none":
        return False
    if fam == "ohem" and not (min_kept >= 0 and thresh == thresh):
        return False
    if fam == "dice":
        cew, dw, smooth = dice
        if not (1 <= C <= LX_MAX_CLASSES and cew >= 0 and dw >= 0 and (cew > 0 or dw > 0) and smooth >= 0):
            return False
    return True


_HW1, _HWN, _HWZ = (1.0, 0.4), (1.0, -0.4), (0.0, 0.4)
_D1 = (1.0, 1.0, 1.0)
# (family, form, N, C, H, W, ignore index, label pattern, logit pattern, class weights, head weights, upstream scalar given, thresh, min_kept,
#  Dice's (ce_weight, dice_weight, smooth), what the row is there for)
_LOSS_ROWS = (
    ("ce", "single", 1, 1, 1, 1, 255, "none", "ordinary", "none", _HW1, False, 0, 0, None, "one pixel of one class: p = 1, loss 0"),
    ("ce", "pair", 1, 2, 3, 5, 255, "tenth", "ordinary", "none", _HW1, True, 0, 0, None, "15 pixels: fewer than a wave"),
    ("ce", "single", 1, 3, 15, 17, 255, "none", "ordinary", "none", _HW1, False, 0, 0, None, "255 pixels, none ignored"),
    ("ce", "pair", 1, 6, 16, 16, -100, "tenth", "confident", "none", _HWN, False, 0, 0, None, "256 pixels: exactly one block; ignore index -100; a negative head weight"),
    ("ce", "single", 1, 7, 1, 257, 255, "allbut1", "ordinary", "none", _HW1, False, 0, 0, None, "257 pixels, one of them labelled"),
    ("ce", "pair", 2, 6, 33, 31, 255, "tenth", "ordinary", "none", _HW1, True, 0, 0, None, "two images of 1023 pixels: block 3 spans both (pixel_of)"),
    ("ce", "single", 3, 8, 5, 17, 3, "tenth", "shift+", "none", _HW1, False, 0, 0, None, "class 3 is the ignore index; logits + 1000; three images inside one block"),
    ("ce", "pair", 2, 9, 33, 31, 255, "tenth", "shift-", "none", _HWZ, False, 0, 0, None, "logits - 1000; a head of weight zero: its gradient is all zeros"),
    ("ce", "single", 2, 16, 9, 7, 255, "tenth", "wide", "none", _HW1, False, 0, 0, None, "own-class logit 60 and 120 below the maximum: p tiny, and exactly 0 in fp32"),
    ("ce", "pair", 1, 17, 11, 13, -100, "none", "constant", "none", _HW1, False, 0, 0, None, "constant map: p = 1 / 17 everywhere"),
    ("ce", "single", 1, 19, 8, 9, 255, "oneclass", "ordinary", "none", _HW1, True, 0, 0, None, "one class present"),
    ("ce", "single", 1, 150, 6, 7, 255, "tenth", "ordinary", "none", _HW1, False, 0, 0, None, "150 classes: the long class loop"),
    ("ce", "pair", 2, 150, 5, 5, 7, "tenth", "wide", "none", _HWN, True, 0, 0, None, "150 classes, wide logits, class 7 ignored"),
    ("ce", "single", 2, 6, 9, 7, 255, "all", "ordinary", "none", _HW1, False, 0, 0, None, "every pixel ignored: loss 0, gradient 0"),
    ("ce", "single", 1, 2, 1025, 1024, 255, "tenth", "ordinary", "none", _HW1, False, 0, 0, None, "1 049 600 pixels: wce_bwd_kernel<1, false> goes round its loop twice"),
    ("wce", "single", 1, 1, 1, 1, 255, "none", "ordinary", "random", _HW1, False, 0, 0, None, "one pixel, one weighted class"),
    ("wce", "pair", 1, 2, 3, 5, 255, "tenth", "ordinary", "random", _HW1, False, 0, 0, None, "15 pixels"),
    ("wce", "single", 1, 3, 5, 51, -100, "tenth", "confident", "onezero", _HW1, False, 0, 0, None, "255 pixels; one class of weight zero"),
    ("wce", "pair", 1, 6, 16, 16, 255, "none", "ordinary", "random", _HWZ, True, 0, 0, None, "256 pixels, none ignored, a head of weight zero"),
    ("wce", "single", 1, 7, 257, 1, 255, "tenth", "ordinary", "zeropresent", _HW1, False, 0, 0, None, "weight zero on every class present: loss 0, gradient 0"),
    ("wce", "pair", 2, 7, 33, 31, 255, "tenth", "ordinary", "random", _HW1, True, 0, 0, None, "a block spans two images"),
    ("wce", "single", 3, 8, 5, 17, 0, "tenth", "shift-", "random", _HW1, False, 0, 0, None, "class 0 is the ignore index; logits - 1000"),
    ("wce", "pair", 2, 9, 7, 9, 255, "allbut1", "shift+", "random", _HWN, False, 0, 0, None, "one labelled pixel, logits + 1000"),
    ("wce", "single", 2, 16, 33, 31, 255, "tenth", "wide", "random", _HW1, True, 0, 0, None, "16 classes, wide logits"),
    ("wce", "pair", 1, 17, 9, 11, 255, "oneclass", "constant", "onezero", _HW1, False, 0, 0, None, "17 classes, constant map, one class present"),
    ("wce", "single", 1, 19, 12, 10, -100, "none", "confident", "random", _HW1, False, 0, 0, None, "19 classes, ignore index -100 and no pixel carries it"),
    ("wce", "pair", 1, 150, 4, 9, 255, "tenth", "ordinary", "random", _HW1, False, 0, 0, None, "150 weighted classes"),
    ("wce", "single", 2, 6, 8, 8, 255, "all", "ordinary", "random", _HW1, False, 0, 0, None, "every pixel ignored"),
    ("wce", "pair", 1, 2, 1025, 1024, 255, "tenth", "ordinary", "random", _HW1, True, 0, 0, None, "1 049 600 pixels: wce_bwd_kernel<2, true> goes round its loop twice"),
    ("ohem", "single", 1, 2, 1, 1, 255, "none", "ordinary", "none", _HW1, False, 0.7, 0, None, "one pixel, min_kept 0"),
    ("ohem", "pair", 1, 3, 3, 5, 255, "tenth", "ordinary", "none", _HW1, False, 0.7, 5, None, "15 pixels"),
    ("ohem", "single", 1, 6, 15, 17, -100, "tenth", "ordinary", "none", _HW1, False, 0.7, 100, None, "255 pixels, ignore index -100"),
    ("ohem", "pair", 1, 7, 16, 16, 255, "none", "confident", "none", _HWN, True, 0.7, 100, None, "256 confident pixels: the k-th smallest p is the threshold"),
    ("ohem", "single", 1, 8, 257, 1, 255, "allbut1", "ordinary", "none", _HW1, False, 0.7, 1, None, "one labelled pixel: min_kept reaches their number"),
    ("ohem", "pair", 2, 6, 33, 31, 255, "tenth", "ordinary", "none", _HW1, True, 0.7, 500, None, "a block spans two images"),
    ("ohem", "single", 2, 9, 33, 31, 4, "tenth", "confident", "none", _HW1, False, 0.7, 500, None, "class 4 is the ignore index"),
    ("ohem", "pair", 3, 16, 5, 17, 255, "tenth", "shift+", "none", _HWZ, False, 0.7, 50, None, "16 classes, logits + 1000, a head of weight zero"),
    ("ohem", "single", 2, 17, 9, 7, 255, "tenth", "wide", "none", _HW1, False, 0.7, 30, None, "17 classes; stored p of exactly 0 sorts first"),
    ("ohem", "single", 1, 19, 8, 9, 255, "oneclass", "shift-", "none", _HW1, True, 0.5, 20, None, "19 classes, one present, logits - 1000"),
    ("ohem", "pair", 1, 150, 6, 7, 255, "tenth", "ordinary", "none", _HW1, False, 0.7, 10, None, "150 classes"),
    ("ohem", "single", 2, 6, 9, 7, 255, "all", "ordinary", "none", _HW1, False, 0.7, 0, None, "every pixel ignored"),
    ("ohem", "single", 2, 3, 33, 31, 255, "tenth", "constant", "none", _HW1, False, 0.1, 10, None, "every pixel tied at p = 1 / 3 > thresh: the threshold is their p, nothing is kept"),
    ("ohem", "pair", 2, 2, 33, 31, 255, "tenth", "grid", "none", _HW1, False, 0.1, 900, None, "logits on a grid of 0.5: min_kept inside a tie group"),
    ("ohem", "single", 1, 3, 200, 180, 255, "tenth", "ordinary", "none", _HW1, False, 0.7, 5000, None, "36 000 pixels: the digit histograms' 128 blocks stride"),
    ("ohem", "pair", 1, 2, 1025, 1024, 255, "tenth", "grid", "none", _HW1, True, 0.6, 300000, None, "1 049 600 pixels: ohem_bwd_kernel goes round its loop twice; every forward grid strides"),
    ("dice", "single", 1, 1, 1, 1, 255, "none", "ordinary", "none", _HW1, False, 0, 0, _D1, "one pixel of one class"),
    ("dice", "pair", 1, 2, 3, 5, 255, "tenth", "ordinary", "none", _HW1, False, 0, 0, _D1, "15 pixels"),
    ("dice", "single", 1, 3, 15, 17, -100, "tenth", "confident", "random", _HW1, False, 0, 0, (1.5, 0.75, 1.0), "255 pixels, class weights, unequal loss weights"),
    ("dice", "pair", 1, 8, 16, 16, 255, "none", "ordinary", "none", _HWN, True, 0, 0, (1.0, 1.0, 0.0), "8 classes: exactly one chunk; smooth 0"),
    ("dice", "single", 1, 9, 1, 257, 255, "tenth", "ordinary", "none", _HW1, False, 0, 0, (1.0, 1.0, 0.0), "9 classes: a second chunk of one class; smooth 0"),
    ("dice", "pair", 2, 7, 33, 31, 255, "tenth", "ordinary", "random", _HW1, True, 0, 0, _D1, "a block spans two images"),
    ("dice", "single", 3, 16, 5, 17, 2, "tenth", "shift+", "none", _HW1, False, 0, 0, _D1, "16 classes: two full chunks; class 2 ignored; logits + 1000"),
    ("dice", "pair", 2, 17, 9, 7, 255, "allbut1", "wide", "onezero", _HWZ, False, 0, 0, _D1, "17 classes: three chunks, the last of one class; one labelled pixel"),
    ("dice", "single", 1, 19, 8, 9, 255, "oneclass", "constant", "none", _HW1, False, 0, 0, (0.5, 2.0, 1.0), "19 classes, constant map, one class present"),
    ("dice", "single", 2, 6, 9, 7, 255, "all", "ordinary", "random", _HW1, False, 0, 0, _D1, "every pixel ignored"),
    ("dice", "single", 2, 6, 33, 31, 255, "tenth", "shift-", "zeropresent", _HW1, False, 0, 0, _D1, "total class weight zero: CE 0, the Dice term alone"),
    ("dice", "pair", 1, 2, 1025, 1024, 255, "tenth", "ordinary", "none", _HW1, False, 0, 0, _D1, "1 049 600 pixels: dice_bwd_kernel goes round its loop twice (LX_BWD_BLOCKS)"),
)


def loss_cases(seed=2313):
    """(id, family, form, N, C, H, W, ignore index, labels, logits, class weights, head weights, upstream, thresh, min_kept, dice, why, seed)"""
    return [("loss-%d" % i,) + row + (seed + i,) for i, row in enumerate(_LOSS_ROWS)]


def _ls_bwd_twice(c):
    return loss_npix(c) > loss_grids(c)[1] * 256


LOSS_REGIMES = [("family: %s" % f, (lambda f_: lambda c: c[1] == f_)(f)) for f in LOSS_FAMILIES] + [
    ("form: %s" % f, (lambda f_: lambda c: c[2] == f_)(f)) for f in LOSS_FORMS] + [
    ("C = %d" % k, (lambda k_: lambda c: c[4] == k_)(k)) for k in (1, 2, 3, 6, 7, 8, 9, 16, 17, 19, 150)] + [
    ("dice: whole class chunks (C % 8 == 0)", lambda c: c[1] == "dice" and c[4] % LX_CHUNK == 0),
    ("dice: several chunks, ragged last", lambda c: c[1] == "dice" and lx_chunks(c[4]) > 1 and c[4] % LX_CHUNK != 0),
] + [("%d pixel%s" % (k, "s" if k > 1 else ""), (lambda k_: lambda c: loss_npix(c) == k_)(k)) for k in (1, 15, 255, 256, 257)] + [
    ("a block spans two images (N >= 2, HW % 256 != 0)", lambda c: c[3] >= 2 and (c[5] * c[6]) % 256 != 0 and loss_npix(c) > 256),
    ("several images inside one block", lambda c: c[3] >= 2 and loss_npix(c) <= 256),
] + [("%s: the forward grid strides" % f, (lambda f_: lambda c: c[1] == f_ and loss_npix(c) > loss_grids(c)[0] * 256)(f)) for f in LOSS_FAMILIES] + [
    ("ohem: the digit histograms' grid strides", lambda c: c[1] == "ohem" and loss_npix(c) > loss_grids(c)[2] * 256),
    ("second trip: wce_bwd_kernel plain, single", lambda c: c[1] == "ce" and c[2] == "single" and _ls_bwd_twice(c)),
    ("second trip: wce_bwd_kernel weighted, pair", lambda c: c[1] == "wce" and c[2] == "pair" and c[10] != "none" and _ls_bwd_twice(c)),
    ("second trip: ohem_bwd_kernel", lambda c: c[1] == "ohem" and _ls_bwd_twice(c)),
    ("second trip: dice_bwd_kernel", lambda c: c[1] == "dice" and _ls_bwd_twice(c)),
] + [("labels: %s" % p, (lambda p_: lambda c: c[8] == p_)(p)) for p in LOSS_LABELS] + [
    ("ignore index 255", lambda c: c[7] == 255),
    ("ignore index -100", lambda c: c[7] == -100),
    ("ignore index inside [0, C)", lambda c: 0 <= c[7] < c[4]),
] + [("logits: %s" % p, (lambda p_: lambda c: c[9] == p_)(p)) for p in LOSS_LOGITS] + [
    ("class weights: %s" % p, (lambda p_: lambda c: c[10] == p_)(p)) for p in LOSS_CW[1:]] + [
    ("head weights (1, 0.4)", lambda c: c[11] == _HW1),
    ("one negative head weight", lambda c: min(c[11]) < 0),
    ("one head weight zero", lambda c: 0.0 in c[11]),
    ("upstream scalar given", lambda c: c[12]),
    ("upstream NULL", lambda c: not c[12]),
    ("ohem: min_kept = 0", lambda c: c[1] == "ohem" and c[14] == 0),
    ("dice: smooth 0", lambda c: c[1] == "dice" and c[15][2] == 0.0),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# the optimizer half of csrc/optim.hip: emrt_grad_clip_scale, emrt_sgd_momentum_step(_sched), emrt_adamw_step through stream_update
# (tests/test_gpu_step_fuzz.py).
# ---------------------------------------------------------------------------------------------------------------------------------
STEP_LONG_MAX_ELEMS = 4 * (8192 * 256 + 1) + 3          # one quad past stream_update's 8192 blocks, plus a 3-element tail
STEP_ENTRIES = ("clip", "sgd", "sgd_sched", "adamw")
STEP_LAYOUTS = ("none", "whole", "quad16", "inquad", "intail", "border", "r32", "adjacent", "empty", "past")
STEP_MIRRORS = ("none", "bf16", "fp16")
STEP_CLIPS = ("below", "above", "zero", "negative", "zerograd")
STEP_NULLS = ("step", "clip_state", "lr_out")
STEP_MAX_RANGES = 32


def clip_grid(n):
    """emrt_grad_clip_scale, optim.hip:292-294"""
    return min(max((n // 4 + 255) // 256, 1), 2048)


def step_grid(n):
    """launch_step, optim.hip:338-340"""
    return min(max((n // 4 + 255) // 256, 1), 8192)


def step_body_tail(n):
    """(n4, tail): quads of the vector body, elements of the scalar tail in block 0.  stream_update, optim.hip:77,124; sqnorm_partial_kernel:30,35"""
    return n // 4, n - n // 4 * 4


def clip_depth(n):
    """fp32 additions in front of one thread's wave_sum in sqnorm_partial_kernel (optim.hip:31-35): four per quad, one for a tail element"""
    n4, tail = step_body_tail(n)
    return 4 * _ceil_div(n4, clip_grid(n) * 256) + (1 if tail else 0)


def fill_step_args_refuses(aligned16, mirror, mirror_aligned8, mirror_dtype, nranges, ranges_given):
    """the refusals of fill_step_args (optim.hip:323-326) for non-null buffers -> the reason or None"""
    if mirror and mirror_dtype not in (1, 2):          # EMRT_BF16, EMRT_F16
        return "the parameter mirror is bf16 or fp16"
    if not aligned16 or (mirror and not mirror_aligned8):
        return "buffers must be 16-byte aligned"
    if nranges < 0 or nranges > STEP_MAX_RANGES or (nranges != 0 and not ranges_given):
        return "0..32 lr-mult ranges"
    return None


def step_ranges(layout, n):
    """the lr-mult ranges [(r0, r1)] of a layout name at n elements.  quad16: all sixteen (start offset, end offset) pairs of the quad pre-test
    `i + 3 >= r0 && i < r1` (optim.hip:104), one range each, two quads apart"""
    n4, tail = step_body_tail(n)
    if layout == "none":
        return []
    if layout == "whole":
        return [(0, n)]
    if layout == "quad16":
        return [(32 * (4 * a + b) + 8 + a, 32 * (4 * a + b) + 20 + b) for a in range(4) for b in range(4)]
    if layout == "inquad":
        return [(41, 43)] if n >= 44 else [(1, min(3, n))]
    if layout == "intail":
        return [(n4 * 4 + (1 if tail == 3 else 0), n)]
    if layout == "border":
        return [(n4 * 4 - 2, n4 * 4 + 2)]
    if layout == "r32":
        return [(16 * i + 1 + i % 4, 16 * i + 6 + i % 3) for i in range(32)]
    if layout == "adjacent":
        return [(8, 13), (13, 22)]
    if layout == "empty":
        return [(9, 9)]
    if layout == "past":
        return [(n, n + 8), (n - 2, n + 5)]
    raise ValueError(layout)


def step_selected(layout, n):
    """sorted element indices inside the union of the ranges, clipped to [0, n)"""
    sel = set()
    for r0, r1 in step_ranges(layout, n):
        sel.update(range(max(r0, 0), min(r1, n)))
    return sorted(sel)


def step_in_domain(c):
    _, entry, n, layout, mirror, nt, clip, nulls, _, _ = c
    if entry not in STEP_ENTRIES or layout not in STEP_LAYOUTS or mirror not in STEP_MIRRORS or nt not in (0, 1) or n < 1:
        return False
    if any(x not in STEP_NULLS for x in nulls):
        return False
    if entry == "clip":
        return clip in STEP_CLIPS and layout == "none" and mirror == "none" and not nulls
    if clip != "":
        return False
    r = step_ranges(layout, n)
    if len(r) > STEP_MAX_RANGES or any(r0 < 0 for r0, _ in r):
        return False
    if layout == "quad16" and n < 32 * 15 + 24:
        return False
    if layout == "intail" and step_body_tail(n)[1] == 0:
        return False
    if layout == "border" and (n < 4 or step_body_tail(n)[1] < 2):
        return False
    return True


# (entry point, n, range layout, mirror, sgd_nt, clip kind, which of step / clip_state / lr_out are NULL, what the row is there for)
_STEP_ROWS = (
    ("clip", 1, "none", "none", 1, "above", (), "one element: the tail alone"),
    ("clip", 3, "none", "none", 1, "below", (), "three tail elements, norm below clip: scale exactly 1"),
    ("clip", 4, "none", "none", 1, "zero", (), "one quad, clip = 0: scale 1"),
    ("clip", 5, "none", "none", 1, "negative", (), "a quad and a tail element, clip < 0: scale 1"),
    ("clip", 4092, "none", "none", 1, "zerograd", (), "1023 quads, all-zero gradient: norm 0, scale 1"),
    ("clip", 4097, "none", "none", 1, "above", (), "1024 quads + 1: four full blocks and one tail element"),
    ("clip", 4102, "none", "none", 1, "below", (), "1025 quads + 2"),
    ("clip", 4095, "none", "none", 1, "above", (), "1023 quads + 3"),
    ("clip", 4096, "none", "none", 1, "zero", (), "1024 quads, clip = 0"),
    ("clip", 4094, "none", "none", 1, "negative", (), "1023 quads + 2, clip < 0"),
    ("clip", 3, "none", "none", 1, "zerograd", (), "an all-zero tail"),
    ("clip", 4 * (2048 * 256 + 1) + 3, "none", "none", 1, "above", (), "2 097 159 elements: sqnorm_partial_kernel's 2048 blocks stride"),
    ("sgd", 1, "none", "none", 1, "", (), "one element: no vector body"),
    ("sgd", 3, "whole", "bf16", 0, "", (), "three tail elements, all inside the range"),
    ("sgd", 4, "whole", "fp16", 1, "", ("lr_out",), "one quad, lr_out NULL"),
    ("sgd", 5, "intail", "none", 1, "", (), "the one tail element is the range"),
    ("sgd", 4092, "quad16", "bf16", 1, "", (), "1023 quads; every start / end offset of the quad pre-test"),
    ("sgd", 4093, "quad16", "none", 0, "", (), "1023 quads + 1, plain loads"),
    ("sgd", 4098, "inquad", "fp16", 1, "", (), "1024 quads + 2; a range inside one quad"),
    ("sgd", 4099, "border", "bf16", 1, "", ("clip_state",), "1024 quads + 3; a range across the body / tail border; clip_state NULL"),
    ("sgd", 4100, "r32", "none", 1, "", (), "1025 quads; 32 ranges"),
    ("sgd", 4103, "intail", "bf16", 0, "", (), "1025 quads + 3; a range inside the tail"),
    ("sgd", 4094, "adjacent", "fp16", 0, "", ("step",), "1023 quads + 2; two adjacent ranges; step NULL"),
    ("sgd", 4101, "empty", "bf16", 1, "", (), "1025 quads + 1; an empty range"),
    ("sgd", 4096, "past", "none", 1, "", (), "1024 quads; a range starting at n and one running past it"),
    ("sgd", STEP_LONG_MAX_ELEMS, "border", "bf16", 1, "", (), "8 388 615 elements: stream_update<1>'s 8192 blocks stride"),
    ("sgd_sched", 4099, "quad16", "bf16", 1, "", (), "the schedule-driven entry point through the same kernel"),
    ("sgd_sched", 4097, "whole", "none", 0, "", STEP_NULLS, "step, clip_state and lr_out all NULL"),
    ("sgd_sched", 5, "past", "fp16", 1, "", (), "five elements, a range past n"),
    ("adamw", 1, "none", "none", 1, "", (), "one element"),
    ("adamw", 3, "whole", "bf16", 1, "", (), "three tail elements"),
    ("adamw", 4, "inquad", "none", 0, "", (), "one quad, a range inside it"),
    ("adamw", 5, "intail", "fp16", 1, "", (), "the one tail element is the range"),
    ("adamw", 4095, "quad16", "bf16", 1, "", (), "1023 quads + 3; every start / end offset"),
    ("adamw", 4096, "r32", "none", 0, "", (), "1024 quads; 32 ranges"),
    ("adamw", 4102, "border", "fp16", 1, "", ("clip_state",), "1025 quads + 2; across the border; clip_state NULL"),
    ("adamw", 4100, "adjacent", "bf16", 1, "", ("lr_out",), "1025 quads; adjacent ranges; lr_out NULL"),
    ("adamw", 4093, "empty", "none", 1, "", ("step",), "1023 quads + 1; an empty range; step NULL"),
    ("adamw", 4101, "past", "bf16", 0, "", (), "1025 quads + 1; ranges at and past n"),
    ("adamw", STEP_LONG_MAX_ELEMS, "intail", "fp16", 1, "", (), "8 388 615 elements: stream_update<2>'s 8192 blocks stride; a range inside the tail"),
)


def step_cases(seed=2414):
    """(id, entry, n, layout, mirror, sgd_nt, clip kind, nulls, why, seed)"""
    return [("step-%d" % i,) + row + (seed + i,) for i, row in enumerate(_STEP_ROWS)]


def _st_quads(c):
    return step_body_tail(c[2])[0]


STEP_REGIMES = [("entry: %s" % e, (lambda e_: lambda c: c[1] == e_)(e)) for e in STEP_ENTRIES] + [
    ("n = %d" % k, (lambda k_: lambda c: c[2] == k_)(k)) for k in (1, 3, 4, 5)] + [
    ("%d quads" % q, (lambda q_: lambda c: _st_quads(c) == q_)(q)) for q in (1023, 1024, 1025)] + [
    ("tail of %d" % t, (lambda t_: lambda c: step_body_tail(c[2])[1] == t_)(t)) for t in (0, 1, 2, 3)] + [
    ("clip: the partial sums' grid strides", lambda c: c[1] == "clip" and _st_quads(c) > clip_grid(c[2]) * 256),
    ("sgd: stream_update's grid strides", lambda c: c[1] == "sgd" and _st_quads(c) > step_grid(c[2]) * 256),
    ("adamw: stream_update's grid strides", lambda c: c[1] == "adamw" and _st_quads(c) > step_grid(c[2]) * 256),
] + [("ranges: %s" % p, (lambda p_: lambda c: c[1] != "clip" and c[3] == p_)(p)) for p in STEP_LAYOUTS] + [
    ("mirror: %s" % p, (lambda p_: lambda c: c[1] != "clip" and c[4] == p_)(p)) for p in STEP_MIRRORS] + [
    ("sgd_nt = %d" % k, (lambda k_: lambda c: c[1] != "clip" and c[5] == k_)(k)) for k in (0, 1)] + [
    ("clip kind: %s" % p, (lambda p_: lambda c: c[6] == p_)(p)) for p in STEP_CLIPS] + [
    ("%s NULL" % p, (lambda p_: lambda c: p_ in c[7])(p)) for p in STEP_NULLS]


# ---------------------------------------------------------------------------------------------------------------------------------
# emrt_segmentation_areas (csrc/optim.hip; tests/test_gpu_step_fuzz.py)
# ---------------------------------------------------------------------------------------------------------------------------------
AREAS_LONG_MAX_ELEMS = 1024 * 4096 + 1
AREAS_LTYPES = (0, 1, 2)          # label_is_int64: 0 = int32, 1 = int64, 2 = uint8


def areas_grid(n):
    """emrt_segmentation_areas, optim.hip:276-277: sixteen labels per thread, at most 1024 blocks"""
    return min((n + 256 * 16 - 1) // (256 * 16), 1024)


def areas_in_domain(c):
    _, ncls, ltype, offset, n, ignore, _, _ = c
    return 1 <= ncls <= 256 and ltype in AREAS_LTYPES and n >= 1 and offset in (0, 1) and (offset == 0 or ltype == 2)


# (classes, label type, byte offset of the uint8 labels, n, ignore index, what the row is there for)
_AREAS_ROWS = (
    (1, 0, 0, 1, 255, "one class, one pixel"),
    (1, 1, 0, 4095, 0, "one class and it is the ignore index: nothing counts"),
    (2, 2, 0, 4096, 255, "uint8 labels, exactly one block's share"),
    (2, 2, 1, 4097, 1, "uint8 at an odd byte offset, a second block of one pixel, class 1 ignored"),
    (19, 0, 0, 4097, 255, "19 classes, int32"),
    (19, 1, 0, 4095, -1, "int64 labels, a negative ignore index that the labels carry"),
    (19, 2, 1, 4096, 255, "uint8 at an odd byte offset"),
    (256, 0, 0, 4096, 300, "256 classes: the whole LDS table; the ignore index above every class"),
    (256, 1, 0, 1, 255, "256 classes, one pixel, class 255 ignored"),
    (256, 2, 0, 4095, 255, "256 classes in uint8: every byte value is a class, 255 ignored"),
    (19, 2, 1, AREAS_LONG_MAX_ELEMS, 255, "4 194 305 pixels: the 1024 blocks stride"),
)


def areas_cases(seed=2515):
    """(id, classes, label type, byte offset, n, ignore index, why, seed)"""
    return [("areas-%d" % i,) + row + (seed + i,) for i, row in enumerate(_AREAS_ROWS)]


AREAS_REGIMES = [("%d class%s" % (k, "es" if k > 1 else ""), (lambda k_: lambda c: c[1] == k_)(k)) for k in (1, 2, 19, 256)] + [
    ("labels: %s" % nm, (lambda t_: lambda c: c[2] == t_)(t)) for t, nm in ((0, "int32"), (1, "int64"), (2, "uint8"))] + [
    ("uint8 at byte offset %d" % o, (lambda o_: lambda c: c[2] == 2 and c[3] == o_)(o)) for o in (0, 1)] + [
    ("n = %d" % k, (lambda k_: lambda c: c[4] == k_)(k)) for k in (1, 4095, 4096, 4097)] + [
    ("the grid strides (n > 1024 x 4096)", lambda c: c[4] > areas_grid(c[4]) * 4096),
    ("ignore index inside [0, ncls)", lambda c: 0 <= c[5] < c[1]),
    ("ignore index outside [0, ncls)", lambda c: not 0 <= c[5] < c[1]),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels that draw a dropout mask, each held to the host model of csrc/drop_hash.hpp (tests/dropout_reference.py) bit for bit:
# emrt_dropout_fwd / emrt_mask_bwd (tests/test_gpu_dropout_fuzz.py), the LayerNorm kernels with a fused branch dropout
# (tests/test_gpu_norm_fuzz.py) and emrt_conv2d_drop (tests/test_gpu_conv_epilogue_fuzz.py)
# ---------------------------------------------------------------------------------------------------------------------------------
DROP_LONG_MAX_ELEMS = 4 * (8192 * 256 + 1)          # one quad past ew_grid's 8192 blocks: the second trip round the grid-stride loop
DROP_PS = (0.0, 2.0 ** -17, 0.1, 0.5, 0.999)          # 0: identity; 2^-17: threshold 0, nothing dropped, the scale still applied
DROP_ARMS = ("mask", "mask+relu", "relu", "stored")          # emrt_mask_bwd: seed + mask alone; seed + relu_out; relu_out alone (p = 0); seed == NULL,
DROP_DTYPES = ("both", "f32", "bf16")                        # p > 0 (relu_out is emrt_conv2d_drop's stored output: both masks)
DROP_SEEDS = (0x0123456789abcdef, 7, 0, 0xfedcba9876543210, 1234 * 0x9E3779B97F4A7C15 % (1 << 63))


def ew_grid(quads):
    """ew_grid (csrc/elementwise.hip): blocks of 256 lanes, at most 8192"""
    return min(max(_ceil_div(quads, 256), 1), 8192)


def drop_n(c):
    """elements of a dropout case: n (element mode) or N hw C (channel mode)"""
    return c[2][0] if c[1] == "element" else c[2][0] * c[2][1] * c[2][2]


def drop_in_domain(c):
    _, mode, dims, p, arms, dtypes, _, _, _ = c
    n = drop_n(c)
    if mode not in ("element", "channel") or n < 4 or n % 4 != 0 or not 0.0 <= p < 1.0 or dtypes not in DROP_DTYPES:
        return False
    if mode == "channel" and (dims[1] < 1 or dims[2] < 1):
        return False
    for arm in arms:          # (emrt_mask_bwd: p == 0 or a seed or relu_out)
        if arm not in DROP_ARMS or (arm == "relu") != (p == 0.0):
            return False
    return True


# (mode, dims, p, arms of emrt_mask_bwd, dtypes, salt, what the row is there for).  element: dims = (n,); channel: dims = (N, hw, C)
_DROP_ROWS = (
    ("element", (4,), 0.0, ("relu",), "both", 1, "one quad, p = 0: the forward is the identity bit for bit, the backward the ReLU mask alone"),
    ("element", (4,), 0.5, ("mask", "stored"), "both", 2, "one quad, one lane"),
    ("element", (1020,), 2.0 ** -17, ("mask",), "both", 3, "255 quads, threshold 0: nothing dropped, every element scaled by 1 / (1 - 2^-17)"),
    ("element", (1020,), 0.1, ("mask+relu",), "both", 4, "255 quads"),
    ("element", (1020,), 0.999, ("mask", "stored"), "both", 5, "255 quads, almost everything dropped, scale 1000"),
    ("element", (1024,), 0.0, ("relu",), "both", 6, "one block exactly, p = 0"),
    ("element", (1024,), 0.1, ("mask", "mask+relu", "stored"), "both", 7, "one block exactly, every arm of the backward with a mask"),
    ("element", (1024,), 0.5, ("mask",), "both", 0, "one block exactly, salt 0"),
    ("element", (1028,), 2.0 ** -17, ("mask+relu", "stored"), "both", 1000, "257 quads: one lane of a second block, threshold 0"),
    ("element", (1028,), 0.5, ("mask", "mask+relu"), "both", 0xFFFFFFFF, "257 quads, the largest salt"),
    ("element", (1028,), 0.999, ("mask+relu",), "both", 11, "257 quads, p = 0.999"),
    ("element", (DROP_LONG_MAX_ELEMS,), 0.5, ("mask",), "bf16", 12, "8 388 612 elements: both kernels go round their grid-stride loop a second time"),
    ("channel", (3, 1, 4), 0.5, ("mask",), "both", 5, "hw = 1, C = 4: three quads, each an image"),
    ("channel", (2, 1, 64), 0.1, ("mask+relu",), "both", 6, "hw = 1"),
    ("channel", (2, 1, 100), 2.0 ** -17, ("mask",), "both", 7, "p = 2^-17: a plane drops only below 2^-17, nothing here; the scale still applied"),
    ("channel", (2, 25, 4), 0.5, ("mask", "mask+relu"), "both", 0, "C = 4: every quad is one pixel; salt 0"),
    ("channel", (4, 25, 64), 0.5, ("mask",), "both", 9, "C hw = 1600: a block of 1024 elements spans two images"),
    ("channel", (3, 25, 100), 0.1, ("mask", "mask+relu"), "both", 10, "C = 100, C hw = 2500: blocks and quads cut across pixels' ends differently in every image"),
    ("channel", (40, 25, 100), 0.999, ("mask",), "both", 11, "p = 0.999, compared in float32: 4000 planes, a handful kept"),
    ("channel", (2, 16, 64), 0.0, ("relu",), "both", 12, "C hw = 1024: an image per block; p = 0"),
    ("channel", (5, 16, 64), 0.5, ("mask+relu",), "both", 13, "C hw = 1024: an image per block"),
)


def drop_cases():
    """(id, mode, dims, p, arms, dtypes, salt, why, seed word of the device): the seed words go round DROP_SEEDS, nothing is drawn"""
    return [("drop-%d" % i,) + row + (DROP_SEEDS[i % len(DROP_SEEDS)],) for i, row in enumerate(_DROP_ROWS)]


DROP_REGIMES = [("%s mode" % m, (lambda m_: lambda c: c[1] == m_)(m)) for m in ("element", "channel")] + [
    ("element: n = %d" % n, (lambda n_: lambda c: c[1] == "element" and c[2][0] == n_)(n)) for n in (4, 1020, 1024, 1028)] + [
    ("element: the second trip (n > 8192 x 1024)", lambda c: c[1] == "element" and c[2][0] // 4 > ew_grid(c[2][0] // 4) * 256),
    ("channel: N > 1, hw = 1", lambda c: c[1] == "channel" and c[2][0] > 1 and c[2][1] == 1),
    ("channel: N > 1, hw = 25", lambda c: c[1] == "channel" and c[2][0] > 1 and c[2][1] == 25),
] + [("channel: C = %d" % k, (lambda k_: lambda c: c[1] == "channel" and c[2][2] == k_)(k)) for k in (4, 64, 100)] + [
    ("channel: C hw % 1024 != 0", lambda c: c[1] == "channel" and (c[2][1] * c[2][2]) % 1024 != 0),
    ("p = 0", lambda c: c[3] == 0.0), ("p = 2^-17 (threshold 0)", lambda c: c[3] == 2.0 ** -17),
] + [("p = %g" % p, (lambda p_: lambda c: c[3] == p_)(p)) for p in (0.1, 0.5, 0.999)] + [
    ("backward arm: %s" % a, (lambda a_: lambda c: a_ in c[4])(a)) for a in DROP_ARMS] + [
    ("channel mode, backward with relu_out", lambda c: c[1] == "channel" and "mask+relu" in c[4]),
    ("seed 0", lambda c: c[8] == 0), ("seed with the top bit set", lambda c: c[8] >> 63 == 1), ("salt 0", lambda c: c[6] == 0)]


# ---- emrt_layernorm_fwd / _bwd with drop_p > 0 -------------------------------------------------------------------------------------
LND_FORMS = ("a+b", "a+b,post", "a+b,qpos", "a+b,addend")          # qpos: layer_norm(q_pos=) also writes q = out + pos; addend: identity_from (dz_addend)
LND_CS = (12, 100, 256, 260, 1000, 1024)


def lnd_in_domain(case):
    _, B, L, C, form, p, salt, max_blocks, rows_knob, _, _ = case
    return C % 4 == 0 and 12 <= C <= 1024 and B * L >= 1 and form in LND_FORMS and 0.0 < p < 1.0 and max_blocks >= 0 and rows_knob >= 0 and salt >= 0


# (B, L, C, form, p, salt, ln_bwd_max_blocks, ln_bwd_rows, what the row is there for)
_LND_ROWS = (
    (1, 1, 12, "a+b", 0.5, 5, 0, 0, "one row of three quads"),
    (3, 7, 12, "a+b,post", 0.1, 6, 0, 0, "21 rows of 12: eight rows share a 256-lane pass"),
    (2, 37, 100, "a+b,qpos", 0.5, 7, 0, 0, "C = 100: 25 quads a row, rows % 4 = 2"),
    (1, 1, 100, "a+b,addend", 0.1, 8, 0, 0, "one row, with the identity's addend"),
    (3, 23, 256, "a+b", 0.1, 11, 0, 0, "C = 256, 69 rows: two backward blocks of 64 rows"),
    (2, 65, 256, "a+b,post", 0.5, 12, 2, 0, "C = 256 under ln_bwd_max_blocks = 2: every backward block loops over its rows"),
    (1, 131, 256, "a+b,qpos", 0.1, 1, 3, 8, "C = 256 under ln_bwd_rows = 8, ln_bwd_max_blocks = 3"),
    (2, 33, 256, "a+b,addend", 0.5, 2, 0, 5, "C = 256 under ln_bwd_rows = 5: 14 blocks of 5 rows, the last of one"),
    (1, 43, 260, "a+b", 0.5, 0, 0, 0, "C = 260: a ragged second pass of one quad; salt 0"),
    (3, 9, 260, "a+b,addend", 0.1, 1000, 0, 7, "C = 260 under ln_bwd_rows = 7"),
    (1, 1, 260, "a+b,qpos", 0.5, 13, 0, 0, "one row of C = 260"),
    (2, 51, 1000, "a+b,post", 0.1, 14, 0, 0, "C = 1000: 250 quads, a ragged fourth pass"),
    (1, 35, 1000, "a+b,qpos", 0.5, 15, 2, 3, "C = 1000 under ln_bwd_rows = 3, ln_bwd_max_blocks = 2"),
    (1, 1, 1000, "a+b", 0.1, 16, 0, 0, "one row of C = 1000"),
    (3, 11, 1024, "a+b,addend", 0.5, 17, 0, 0, "C = 1024: four whole passes"),
    (1, 67, 1024, "a+b", 0.1, 18, 2, 0, "C = 1024 under ln_bwd_max_blocks = 2"),
    (2, 3, 1024, "a+b,post", 0.5, 0xFFFFFFFF, 0, 4, "C = 1024 under ln_bwd_rows = 4; the largest salt"),
)


def lnd_cases(seed=2717):
    """(id, B, L, C, form, p, salt, ln_bwd_max_blocks, ln_bwd_rows, why, seed)"""
    return [("lnd-%d" % i,) + row + (seed + i,) for i, row in enumerate(_LND_ROWS)]


LND_REGIMES = [("C = %d" % k, (lambda k_: lambda c: c[3] == k_)(k)) for k in LND_CS] + [
    ("rows % 4 != 0", lambda c: (c[1] * c[2]) % 4 != 0), ("rows = 1", lambda c: c[1] * c[2] == 1),
] + [("form ln(%s)" % f, (lambda f_: lambda c: c[4] == f_)(f)) for f in LND_FORMS] + [
    ("p = %g" % p, (lambda p_: lambda c: c[5] == p_)(p)) for p in (0.1, 0.5)] + [
    ("backward under the default knobs", lambda c: c[7] == 0 and c[8] == 0),
    ("backward under ln_bwd_rows", lambda c: c[8] > 0),
    ("backward under ln_bwd_max_blocks", lambda c: c[7] > 0),
    ("backward blocks loop under the block cap", lambda c: ln_bwd_blocks(c[1] * c[2], c[3], c[8], c[7])[1]),
    ("several backward blocks", lambda c: ln_bwd_blocks(c[1] * c[2], c[3], c[8], c[7])[0] > 1)]


# ---- emrt_conv2d_drop: dropout(relu(x w + bias)) drawn in the 64x64 tile's epilogue ------------------------------------------------
CDROP_MS = (1, 63, 64, 65, 114)
CDROP_CS = (8, 64, 264)
CDROP_OCS = (8, 72, 96, 1024)


def conv_drop_vec_ok(M, C, ldin, OC, ldout, esz, in_al=True, out_al=True):
    """Mirrors what emrt_conv2d_drop asks (csrc/conv.hip): conv_is_vec of the input and conv_plan's vec_out of the output; anything else is refused"""
    epc = 16 // esz
    vec_in = C % epc == 0 and ldin % epc == 0 and (M * ldin) % epc == 0 and in_al
    vec_out = out_al and ldout % epc == 0 and (M * ldout) % epc == 0 and OC % 8 == 0
    return vec_in and vec_out


def cdrop_in_domain(c):
    _, M, C, ldin, OC, ldout, p, _, _, _ = c
    if not (M > 0 and C > 0 and OC > 0 and OC % 8 == 0 and M * OC < 1 << 32 and 0.0 < p < 1.0 and ldin >= C and ldout >= OC):
        return False
    return all(conv_drop_vec_ok(M, C, ldin, OC, ldout, esz) for esz in (4, 2))          # every case runs in fp32 and in bf16


# (M, C, ldin, OC, ldout, p, salt, what the row is there for)
_CDROP_ROWS = (
    (1, 8, 8, 8, 8, 0.5, 5, "one row, one group of 8"),
    (1, 64, 64, 72, 72, 0.1, 6, "one row of nine groups"),
    (63, 8, 8, 96, 96, 0.5, 7, "one ragged M tile, two N tiles (the second of 32 columns)"),
    (63, 264, 264, 72, 80, 0.1, 8, "ldout > OC: rows of 80 hold a slice of 72"),
    (64, 64, 64, 8, 8, 0.5, 0, "one whole M tile, an N tile of one group; salt 0"),
    (64, 8, 16, 1024, 1024, 0.1, 11, "sixteen N tiles; ldin > C"),
    (65, 64, 64, 96, 96, 0.1, 12, "a second M tile of one row"),
    (65, 264, 264, 8, 24, 0.5, 13, "ldout = 3 OC"),
    (114, 64, 72, 72, 72, 0.5, 14, "114 rows, ldin > C: OC = 72 makes (m * OC + n0) >> 3 differ from (m * ldout + n0) >> 3 only where ldout != OC"),
    (114, 264, 264, 1024, 1032, 0.1, 1000, "114 x 1024 in rows of 1032"),
    (114, 8, 8, 96, 128, 0.5, 0xFFFFFFFF, "ldout = 128 > OC = 96; the largest salt"),
    (64, 264, 264, 72, 72, 0.1, 15, "K = 264: five k-tiles in bf16, a ragged last one"),
)


def cdrop_cases(seed=2818):
    """(id, M, C, ldin, OC, ldout, p, salt, why, seed)"""
    return [("cdrop-%d" % i,) + row + (seed + i,) for i, row in enumerate(_CDROP_ROWS)]


CDROP_REGIMES = [("M = %d" % k, (lambda k_: lambda c: c[1] == k_)(k)) for k in CDROP_MS] + [
    ("C = %d" % k, (lambda k_: lambda c: c[2] == k_)(k)) for k in CDROP_CS] + [
    ("OC = %d" % k, (lambda k_: lambda c: c[4] == k_)(k)) for k in CDROP_OCS] + [
    ("ldout == OC", lambda c: c[5] == c[4]), ("ldout > OC (a slice of a wider buffer)", lambda c: c[5] > c[4]), ("ldin > C", lambda c: c[3] > c[2]),
    ("ragged last M tile", lambda c: c[1] % 64 != 0), ("several M tiles", lambda c: c[1] > 64), ("several N tiles", lambda c: c[4] > 64),
    ("ragged last N tile", lambda c: c[4] % 64 != 0),
] + [("p = %g" % p, (lambda p_: lambda c: c[6] == p_)(p)) for p in (0.1, 0.5)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the small streaming kernels of csrc/elementwise.hip (tests/test_gpu_elementwise_fuzz.py): emrt_add, emrt_add_f32row,
# emrt_add_f32row_levels, emrt_add3d, emrt_acc3d, emrt_concat_tokens, emrt_cast, emrt_sigmoid_fwd / _bwd, emrt_memcpy (memcpy_kernel = 1)
# ---------------------------------------------------------------------------------------------------------------------------------
EW_TRIP = 8192 * 256 + 1          # quads (lanes) of the one second-trip case of each kernel: one past ew_grid's 8192 blocks of 256
EW_LONG_MAX_ELEMS = 4 * EW_TRIP
EW_MEMCPY_TRIP = 2048 * 256 * 16 + 16          # bytes: copy16_kernel's grid stops at 2048 blocks
EW_KERNELS = ("add", "add_f32row", "levels", "add3d", "acc3d", "concat", "split", "cast_to", "cast_from", "sigmoid_fwd", "sigmoid_bwd", "memcpy")
EW_DTYPES = ("f32", "bf16", "f16")
EW_VIEWS = ("dense", "slab", "slice")          # slab: tokens [:, s:s + n] of [B, Lv, C]; slice: channels [c0:c0 + C] of a wider map


def ew_lanes(c):
    """lanes (quads, or elements of the scalar kernels, or 16-byte words of the copy) a case's grid-stride loop covers"""
    k, s = c[1], c[3]
    if k in ("add", "add_f32row"):
        return s[0] // 4
    if k == "levels":
        return sum(s[0]) * s[1] // 4
    if k in ("add3d", "acc3d"):
        return s[0] * s[1] * s[2] // 4
    if k in ("concat", "split"):
        return s[0] * s[1] * sum(s[2]) // 4
    if k == "memcpy":
        return s[0] // 16
    return s[0]


def ew_second_trip(c):
    if c[1] == "memcpy":
        return c[3][0] % 16 == 0 and c[3][1] == 0 and ew_lanes(c) > 2048 * 256
    return ew_lanes(c) > ew_grid(ew_lanes(c)) * 256


def ew_in_domain(c):
    _, k, d, s, _, _ = c
    if k not in EW_KERNELS:
        return False
    if d not in (EW_DTYPES if k not in ("sigmoid_fwd", "sigmoid_bwd", "memcpy") else ("f32",)):
        return False
    if k in ("cast_to", "cast_from"):
        return d in ("bf16", "f16") and s[0] >= 1
    if k in ("add", "add_f32row"):
        n, period = s
        return n > 0 and n % 4 == 0 and period > 0 and period % 4 == 0 and period <= n
    if k == "levels":
        sizes, C = s
        return 1 <= len(sizes) <= 4 and all(x > 0 for x in sizes) and C > 0 and C % 4 == 0
    if k in ("add3d", "acc3d"):
        B, rows, cols = s[:3]
        return B > 0 and rows > 0 and cols > 0 and cols % 4 == 0 and all(v in EW_VIEWS for v in s[3:]) and len(s) == (6 if k == "add3d" else 5)
    if k in ("concat", "split"):
        B, C, parts = s
        return B > 0 and C > 0 and C % 4 == 0 and 1 <= len(parts) <= 8 and all(x > 0 for x in parts)
    if k == "memcpy":
        return s[0] > 0 and s[1] in (0, 4, 8)
    return s[0] >= 1


def _ew_rows():
    """(kernel, dtype, shape, what the row is there for); shape per kernel: add / add_f32row (n, period); levels ((rows of each level), C);
    add3d (B, rows, cols, view of a, of b, of out); acc3d (B, rows, cols, view of dst, of src); concat / split (B, C, (tokens of each part));
    cast_to / cast_from (n,); sigmoid_* (n,); memcpy (bytes, byte offset of both pointers off a 16-byte boundary)"""
    rows = []
    every = lambda k, s, why: rows.extend((k, d, s, why) for d in EW_DTYPES)
    for k in ("add", "add_f32row"):
        every(k, (4, 4), "one lane: period == n == 4")
        every(k, (1020, 1020), "255 quads, period == n")
        every(k, (1020, 4), "255 quads, period 4: every quad reads the same one")
        every(k, (1020, 340), "255 quads, a period that divides n")
        every(k, (1020, 16), "255 quads, a period that does not divide n")
        every(k, (1024, 1024), "256 quads, period == n")
        every(k, (1024, 256), "256 quads, a period that divides n")
        every(k, (1024, 48), "256 quads, a period that does not divide n")
        every(k, (1028, 1028), "257 quads, period == n")
        every(k, (1028, 4), "257 quads, period 4")
        every(k, (1028, 24), "257 quads, a period that does not divide n")
        rows.append((k, "bf16", (EW_LONG_MAX_ELEMS, 4000), "the second trip; a period that does not divide n"))
    every("levels", ((1,), 4), "L = 1, one row, one lane")
    every("levels", ((7,), 100), "L = 1")
    every("levels", ((5, 1), 100), "L = 2, the last level of one row")
    every("levels", ((1, 9), 256), "L = 2, the first level of one row")
    every("levels", ((3, 9, 1), 256), "L = 3, the last level of one row")
    every("levels", ((4, 1, 6), 4), "L = 3, the middle level of one row")
    every("levels", ((1, 6, 2, 1), 4), "L = 4, first and last level of one row")
    every("levels", ((64, 1, 17, 3), 100), "L = 4, C = 100")
    every("levels", ((200, 55), 4), "255 quads")
    every("levels", ((256,), 4), "256 quads")
    every("levels", ((1, 255, 1), 4), "257 quads")
    rows.append(("levels", "bf16", ((2097000, 1, 152), 4), "the second trip: 2 097 153 rows of one quad, a level of one row in the middle"))
    for k, nv in (("add3d", 3), ("acc3d", 2)):
        dense = ("dense",) * nv
        every(k, (1, 1, 4) + dense, "one lane: B = 1, rows = 1")
        every(k, (3, 5, 68) + dense, "255 quads, all dense")
        every(k, (2, 8, 64) + dense, "256 quads, all dense")
        every(k, (1, 257, 4) + dense, "257 quads, B = 1")
        for i in range(nv):
            for v in ("slab", "slice"):
                views = tuple(v if j == i else "dense" for j in range(nv))
                every(k, (3, 5, 68) + views, "operand %d is a %s, the others dense" % (i, v))
        every(k, (2, 7, 36) + ("slab", "slice", "slab")[:nv], "every operand strided")
        every(k, (2, 7, 36) + ("slice", "slab", "slice")[:nv], "every operand strided, the other way round")
        every(k, (1, 9, 20) + ("slice",) * nv, "B = 1, channel slices")
        every(k, (3, 1, 12) + ("slab",) * nv, "rows = 1, token slabs")
        rows.append((k, "bf16", (1, EW_TRIP, 4) + dense, "the second trip"))
    for k in ("concat", "split"):
        every(k, (1, 4, (1,)), "one part of one token, one lane")
        every(k, (3, 64, (7,)), "one part")
        every(k, (1, 64, (1, 4, 9, 36)), "4 parts, a part of one token first (the pyramid-pooling tokens)")
        every(k, (3, 4, (36, 9, 4, 1)), "4 parts, a part of one token last")
        every(k, (3, 64, (5, 1, 3, 2)), "4 parts, a part of one token in the middle")
        every(k, (1, 4, (1, 2, 3, 4, 5, 6, 7, 8)), "8 parts, a part of one token first")
        every(k, (3, 64, (2, 1, 2, 1, 3, 1, 2, 1)), "8 parts, parts of one token in the middle and last")
        every(k, (3, 4, (50, 35)), "255 quads")
        every(k, (1, 4, (255, 1)), "256 quads")
        every(k, (1, 4, (1, 256)), "257 quads")
        rows.append((k, "bf16", (1, 4, (2097152, 1)), "the second trip; the last part is the one token past the grid"))
    for k in ("cast_to", "cast_from"):
        for d in ("bf16", "f16"):
            for n in (1, 3, 255, 257):
                rows.append((k, d, (n,), "n = %d (no multiple-of-4 rule)" % n))
        rows.append((k, "f16" if k == "cast_to" else "bf16", (EW_TRIP,), "the second trip"))
    for k in ("sigmoid_fwd", "sigmoid_bwd"):
        rows.append((k, "f32", (1,), "one element"))
        rows.append((k, "f32", (257,), "a second block of one element"))
        rows.append((k, "f32", (2443,), "the grid over [-30, 30] and +-100"))
        rows.append((k, "f32", (EW_TRIP,), "the second trip"))
    rows.append(("memcpy", "f32", (16, 0), "16 bytes: one lane"))
    rows.append(("memcpy", "f32", (4096 + 16, 0), "257 lanes"))
    rows.append(("memcpy", "f32", (24, 0), "a size that is no multiple of 16: the runtime's copy"))
    rows.append(("memcpy", "f32", (4096 + 8, 0), "4104 bytes: the runtime's copy"))
    rows.append(("memcpy", "f32", (32, 4), "pointers 4 bytes off a 16-byte boundary: the runtime's copy"))
    rows.append(("memcpy", "f32", (4096, 8), "pointers 8 bytes off: the runtime's copy"))
    rows.append(("memcpy", "f32", (EW_MEMCPY_TRIP, 0), "8 388 624 bytes: copy16_kernel's 2048 blocks stride"))
    return rows


def ew_cases(seed=2919):
    """(id, kernel, dtype, shape, why, seed)"""
    return [("ew-%d" % i,) + row + (seed + i,) for i, row in enumerate(_ew_rows())]


def _ew_is(k):
    return lambda c: c[1] == k


def _ew_period(kind):
    def pred(c):
        if c[1] not in ("add", "add_f32row") or ew_second_trip(c):
            return False
        n, period = c[3]
        return {"== n": period == n, "4": period == 4 and n > 4, "divides n": 4 < period < n and n % period == 0, "does not divide n": n % period != 0}[kind]
    return pred


EW_REGIMES = [("kernel: %s, %s" % (k, d), (lambda k_, d_: lambda c: c[1] == k_ and c[2] == d_)(k, d)) for k in EW_KERNELS for d in EW_DTYPES
              if not (k in ("sigmoid_fwd", "sigmoid_bwd", "memcpy") and d != "f32") and not (k in ("cast_to", "cast_from") and d == "f32")] + [
    ("second trip: %s" % k, (lambda k_: lambda c: c[1] == k_ and ew_second_trip(c))(k)) for k in EW_KERNELS] + [
    ("%d lane%s" % (q, "s" if q > 1 else ""), (lambda q_: lambda c: c[1] != "memcpy" and ew_lanes(c) == q_)(q)) for q in (1, 255, 256, 257)] + [
    ("add: period %s" % kd, _ew_period(kd)) for kd in ("== n", "4", "divides n", "does not divide n")] + [
    ("levels: L = %d" % l, (lambda l_: lambda c: c[1] == "levels" and len(c[3][0]) == l_)(l)) for l in (1, 2, 3, 4)] + [
    ("levels: a level of one row", lambda c: c[1] == "levels" and 1 in c[3][0]),
    ("levels: the last level of one row", lambda c: c[1] == "levels" and len(c[3][0]) > 1 and c[3][0][-1] == 1),
] + [("levels: C = %d" % k, (lambda k_: lambda c: c[1] == "levels" and c[3][1] == k_)(k)) for k in (4, 100, 256)] + [
    ("%s: operand %d a %s, the others dense" % (k, i, v),
     (lambda k_, i_, v_: lambda c: c[1] == k_ and c[3][3 + i_] == v_ and all(x == "dense" for j, x in enumerate(c[3][3:]) if j != i_))(k, i, v))
    for k, nv in (("add3d", 3), ("acc3d", 2)) for i in range(nv) for v in ("slab", "slice")] + [
    ("%s: every operand strided" % k, (lambda k_: lambda c: c[1] == k_ and "dense" not in c[3][3:])(k)) for k in ("add3d", "acc3d")] + [
    ("%s: B = 1" % k, (lambda k_: lambda c: c[1] == k_ and c[3][0] == 1 and not ew_second_trip(c))(k)) for k in ("add3d", "acc3d")] + [
    ("%s: rows = 1" % k, (lambda k_: lambda c: c[1] == k_ and c[3][1] == 1)(k)) for k in ("add3d", "acc3d")] + [
    ("%s: %d part%s" % (k, n, "s" if n > 1 else ""), (lambda k_, n_: lambda c: c[1] == k_ and len(c[3][2]) == n_ and not ew_second_trip(c))(k, n))
    for k in ("concat", "split") for n in (1, 4, 8)] + [
    ("concat / split: a part of one token %s" % w, (lambda w_: lambda c: c[1] in ("concat", "split") and len(c[3][2]) > 1 and {
        "first": c[3][2][0] == 1, "last": c[3][2][-1] == 1, "in the middle": 1 in c[3][2][1:-1]}[w_])(w)) for w in ("first", "last", "in the middle")] + [
    ("concat / split: B = %d" % b, (lambda b_: lambda c: c[1] in ("concat", "split") and c[3][0] == b_)(b)) for b in (1, 3)] + [
    ("concat / split: C = %d" % k, (lambda k_: lambda c: c[1] in ("concat", "split") and c[3][1] == k_)(k)) for k in (4, 64)] + [
    ("cast: n = %d" % n, (lambda n_: lambda c: c[1] in ("cast_to", "cast_from") and c[3][0] == n_)(n)) for n in (1, 3, 255, 257)] + [
    ("memcpy: the copy kernel", lambda c: c[1] == "memcpy" and c[3][0] % 16 == 0 and c[3][1] == 0),
    ("memcpy: a size that is no multiple of 16", lambda c: c[1] == "memcpy" and c[3][0] % 16 != 0),
    ("memcpy: misaligned pointers", lambda c: c[1] == "memcpy" and c[3][1] != 0)]


# ---------------------------------------------------------------------------------------------------------------------------------
CASES = {
    "batchnorm": bn_cases(), "groupnorm": gn_cases(), "groupnorm_levels": gnl_cases(), "layernorm": ln_cases(),
    "resize": resize_cases(), "maxpool": maxpool_cases(), "adaptive_pool": adaptive_cases(), "pyramid": pyramid_cases(),
    "mha": mha_cases(), "msda": msda_cases(), "gconv": gconv_cases(), "conv": conv_cases(),
    "loss": loss_cases(), "step": step_cases(), "areas": areas_cases(),
    "dropout": drop_cases(), "layernorm_drop": lnd_cases(), "conv_drop": cdrop_cases(), "elementwise": ew_cases(),
}
REGIMES = {
    "batchnorm": BN_REGIMES, "groupnorm": GN_REGIMES, "groupnorm_levels": GNL_REGIMES, "layernorm": LN_REGIMES,
    "resize": RESIZE_REGIMES, "maxpool": MAXPOOL_REGIMES, "adaptive_pool": ADAPTIVE_REGIMES, "pyramid": PYRAMID_REGIMES,
    "mha": MHA_REGIMES, "msda": MSDA_REGIMES, "gconv": GCONV_REGIMES, "conv": CONV_REGIMES,
    "loss": LOSS_REGIMES, "step": STEP_REGIMES, "areas": AREAS_REGIMES,
    "dropout": DROP_REGIMES, "layernorm_drop": LND_REGIMES, "conv_drop": CDROP_REGIMES, "elementwise": EW_REGIMES,
}
IN_DOMAIN = {
    "batchnorm": bn_in_domain, "groupnorm": gn_in_domain, "groupnorm_levels": gnl_in_domain, "layernorm": ln_in_domain,
    "resize": resize_in_domain, "maxpool": maxpool_in_domain, "adaptive_pool": adaptive_in_domain, "pyramid": pyramid_in_domain,
    "mha": mha_in_domain, "msda": msda_in_domain, "gconv": gconv_in_domain, "conv": conv_in_domain,
    "loss": loss_in_domain, "step": step_in_domain, "areas": areas_in_domain,
    "dropout": drop_in_domain, "layernorm_drop": lnd_in_domain, "conv_drop": cdrop_in_domain, "elementwise": ew_in_domain,
}


# cases a regime must keep: two, except where the sweep asks for exactly one.  gconv: a block goes round its tile loop twice only from
# 4097 tiles (257 x 257 pixels) or, with statistics, from 2049 / nslices: one case each, under GCONV_LONG_MAX_ELEMS
REGIME_MIN = {("maxpool", "k = 7"): 1, ("msda", "dref on a band pyramid (GRAD_GLOBAL)"): 1,
              ("gconv", "grid-stride: forward, no statistics"): 1, ("gconv", "grid-stride: forward with statistics"): 1, ("gconv", "grid-stride: dgrad"): 1,
              # conv: one case each shows that a refused kernel's problem reaches the ladder's own kernel (the issue asks for exactly one)
              ("conv", "8p asked, refused by igemm8p_ok: the ladder's kernel"): 1, ("conv", "thin shape refused by thin_bwd_ok"): 1,
              ("conv", "xk: fewer k-tiles than the copies asked for"): 1,
              # loss / step / areas: one case each above the ordinary size cap sends a kernel round its grid-stride loop a second time
              ("loss", "ce: the forward grid strides"): 1, ("loss", "wce: the forward grid strides"): 1, ("loss", "ohem: the forward grid strides"): 1,
              ("loss", "dice: the forward grid strides"): 1, ("loss", "second trip: wce_bwd_kernel plain, single"): 1,
              ("loss", "second trip: wce_bwd_kernel weighted, pair"): 1, ("loss", "second trip: ohem_bwd_kernel"): 1,
              ("loss", "second trip: dice_bwd_kernel"): 1,
              ("step", "clip: the partial sums' grid strides"): 1, ("step", "sgd: stream_update's grid strides"): 1,
              ("step", "adamw: stream_update's grid strides"): 1, ("areas", "the grid strides (n > 1024 x 4096)"): 1,
              # dropout / elementwise: one case per kernel above the ordinary size cap, the second trip round its grid-stride loop
              ("dropout", "element: the second trip (n > 8192 x 1024)"): 1}
REGIME_MIN.update({("elementwise", "second trip: %s" % k): 1 for k in EW_KERNELS})


def regime_hits(op):
    """[(regime, [ids of the cases that hit it])]"""
    return [(name, [c[0] for c in CASES[op] if pred(c)]) for name, pred in REGIMES[op]]


def regime_table():
    """the table of the module docstring, one line per regime"""
    lines = []
    for op in CASES:
        for name, ids in regime_hits(op):
            short = sorted(int(i.rsplit("-", 1)[1]) for i in ids)
            lines.append("  %-17s %-50s %s-{%s}" % (op, name, ids[0].rsplit("-", 1)[0] if ids else "", ",".join(str(s) for s in short)))
    return "\n".join(lines)
