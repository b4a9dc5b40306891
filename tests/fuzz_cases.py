"""Seeded random case lists for the shape sweeps of csrc/norm.hip, csrc/spatial.hip and the inference glue
(tests/test_gpu_norm_fuzz.py, tests/test_gpu_spatial_fuzz.py, tests/test_gpu_infer_glue.py) and of csrc/attn.hip
(tests/test_gpu_mha_fuzz.py; its float64 reference and bounds are tests/mha_reference.py), the written-out case list of the sweep of
csrc/msda.hip by plan, build and layout (tests/test_gpu_msda_fuzz.py; tests/msda_reference.py), the written-out case list of the sweep of
csrc/gconv.hip by group shape, launch plan and view (tests/test_gpu_gconv_fuzz.py), and the dispatchers' shape predicates
restated in Python.  No GPU and no library import: tests/test_fuzz_cases_cpu.py checks on any machine that every case lies inside its
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

Not reachable through the wrappers, on purpose:
  * functional.pyramid_tokens_to_maps passes align_corners=True to both pyramid entry points (the model's only use), so the pyramid sweep
    draws no align_corners=False case; the per-scale resize kernels see both conventions in the resize sweep.
  * the 64-bit index branch of unravel3 / unravel4 (csrc/common.hpp) needs more than 2^32 elements and stays unexercised.
  * msda: the refusals (rows too long for a scatter slab, L = 2, dref with M != 8) are pinned by tests/test_msda_plan_cpu.py and stay out
    of the sweep; FINALIZE and the band kinds do not exist for the (1, 4) build (see MSDA_REGIMES).
  * gconv: emrt_gconv2d has no dilation and no kernel size but 3; maps of 2^31 pixels and more are refused (check_common).  The refusals
    are one separate test without a launch (tests/test_gpu_gconv_fuzz.py).
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
CASES = {
    "batchnorm": bn_cases(), "groupnorm": gn_cases(), "groupnorm_levels": gnl_cases(), "layernorm": ln_cases(),
    "resize": resize_cases(), "maxpool": maxpool_cases(), "adaptive_pool": adaptive_cases(), "pyramid": pyramid_cases(),
    "mha": mha_cases(), "msda": msda_cases(), "gconv": gconv_cases(),
}
REGIMES = {
    "batchnorm": BN_REGIMES, "groupnorm": GN_REGIMES, "groupnorm_levels": GNL_REGIMES, "layernorm": LN_REGIMES,
    "resize": RESIZE_REGIMES, "maxpool": MAXPOOL_REGIMES, "adaptive_pool": ADAPTIVE_REGIMES, "pyramid": PYRAMID_REGIMES,
    "mha": MHA_REGIMES, "msda": MSDA_REGIMES, "gconv": GCONV_REGIMES,
}
IN_DOMAIN = {
    "batchnorm": bn_in_domain, "groupnorm": gn_in_domain, "groupnorm_levels": gnl_in_domain, "layernorm": ln_in_domain,
    "resize": resize_in_domain, "maxpool": maxpool_in_domain, "adaptive_pool": adaptive_in_domain, "pyramid": pyramid_in_domain,
    "mha": mha_in_domain, "msda": msda_in_domain, "gconv": gconv_in_domain,
}


# cases a regime must keep: two, except where the sweep asks for exactly one.  gconv: a block goes round its tile loop twice only from
# 4097 tiles (257 x 257 pixels) or, with statistics, from 2049 / nslices: one case each, under GCONV_LONG_MAX_ELEMS
REGIME_MIN = {("maxpool", "k = 7"): 1, ("msda", "dref on a band pyramid (GRAD_GLOBAL)"): 1,
              ("gconv", "grid-stride: forward, no statistics"): 1, ("gconv", "grid-stride: forward with statistics"): 1, ("gconv", "grid-stride: dgrad"): 1}


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
