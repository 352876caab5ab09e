// mcs_fa_macros.h — the hand-scheduled gfx950 pieces shared by the FIFO decision loop
// (mcs_fifo_asm.hip) and the DELAY loop (mcs_delay_asm.hip): the fixed register map, the node
// formats' fit tests, commits, slot inserts, releases and record handling.  Included by .hip files
// only (inline-asm text).
#pragma once

// ---- gfx950 hazard audit of the hand-scheduled loops (FIFO W16R/W16S/fused, DELAY) ----------------
// LLVM's hazard recognizer does not look inside inline asm, so every producer -> consumer pair the
// hardware does not interlock is covered here by instruction distance or an explicit s_nop.  A
// "wait state" is one issued instruction of this wave (s_nop N = N + 1 of them).
//
//  hazard (CDNA3/gfx950)                           needs  where it occurs                     covered by
//  VALU writes VGPR -> DPP reads it                  2     every DPP min/max chain (SCANEND,   s_nop 1 between the steps; before
//                                                          W16C's MCS_FC_WMIN, the DELAY       the first: s_nop 1, or (DELAY rel)
//                                                          filter)                             s_mov s96 + s_nop 0
//                                                          W16C's shifted record columns       v94's write, three v_mov and s_nop 1
//                                                          (MCS_FC_SHIFT: v_mov_b32_dpp        before the first; v95 / v96 are
//                                                          wave_shl:1 of v94, v95, v96)        written earlier still
//  SDWA / op_sel write preserving the other word     1     MCS_FA_FIT16: v80/v81 (WORD_1,      v_cmp_lt s[60:61] + v_ffbl v117
//    -> VALU reads that VGPR (DstSelForwarding)            UNUSED_PRESERVE) -> v_perm          between (found by measurement,
//                                                                                              tools/asm_debug.py)
//                                                          MCS_FA_FITBITS16C: v86 (WORD_0,     the second v_perm (v81) between the
//                                                          then WORD_1 UNUSED_PRESERVE, which  two writes; the caller's scalar
//                                                          reads the first write) -> v_cmp     instruction (the pass: s_add s55,
//                                                                                              the release tail: s_cmp_le_u32)
//                                                                                              between the second and the v_cmp
//  VALU writes SGPR -> v_readlane / v_writelane      4     none: every lane select is SALU-    (s50/s85/s82 from s_ff1, s47/m0
//    uses it as the lane select                            written                             from s_add/s_mov)
//  SALU writes M0 -> v_writelane with an M0 lane     1*    result writes at a Level0 decision  >= 1 other instruction between
//    select (*not in the ISA table; kept anyway)           (HEAD, ZEROKX)                      (s_add s80 / s_ff1, s_lshl3_add)
//                                                          DELAY G list (MCS_FD_ENUM: m0 =     s_add s86 between
//                                                          cursor -> v_writelane v113/v118)
//                                                          W16C's record read (MCS_FC_RECNEXT: s_add s80 + two v_writelane between,
//                                                          v_readlane with m0 the lane select;  in the waiting-head section s_add s82
//                                                          the pass, the waiting-head section   and s_mov s43 more; after mcsfa_zero
//                                                          and mcsfa_zhead alike)               the two v_writelane at least
//  VALU writes VGPR -> v_readlane / v_readfirstlane  1     DECIDE16R / DECIDE16C / ZEROKX      >= 3 instructions between every
//    reads it (gfx950)                                     read v86, v117; REC16 after TAKE16; pair; SCANEND, WMIN: s_nop 1;
//                                                          SCANEND, MCS_FC_WMIN v120;          v87: a batch's passes apart
//                                                          MCS_FC_ZROUTE v87 (written at the
//                                                          batch's TAKE16C)
//                                                          W16C's v89 / v90 / v107 (written    s_mov s47 + three v_readlane after
//                                                          per batch only, MCS_FC_SHIFT)       the batch's
//                                                          W16C's sections: v72-v75, v80, v81,  the pass's own distances (the same
//                                                          v86 of MCS_FA_FITBITS16C in the tail macros: FITBITS16C, DECIDE16C)
//                                                          DELAY G pass (r04): v_cndmask v113  >= 6 (GTEST's scalar prologue)
//                                                          -> GTEST's v_readlane v113; v123
//                                                          (indexed move) -> v_readlane s74     >= 3 (s_set_gpr_idx_off, s_add,
//                                                                                              s_cmp)
//  VALU writes VCC -> s_cbranch_vccz/vccnz           0     ANYFIT -> the fit branch; W16C's    (interlocked on gfx9; the pass's
//                                                          row and LIVE compares (v_cmp vcc,   head and the compares branch
//                                                          then s_cbranch_vccz / vccnz: copies, right after the v_cmp)
//                                                          scan, sleep chain, bulk move)
//  VALU writes EXEC -> DPP (5) / v_readlane (4)      5/4   none: exec is written by SALU only   (no v_cmpx in any loop; W16C's row
//                                                                                              blocks: s_mov_b64 exec; its
//                                                                                              commit leaves exec alone)
//  SALU writes an SGPR pair -> VALU reads it as a    0     DECIDE16C: s_lshl_b64 s[60:61] ->    (interlocked; four scalar
//    lane mask (v_cndmask)                                 the indexed v_cndmask               instructions lie between anyway)
//  VMEM store of > 64 bits -> its data VGPRs         1     none: every store is one dword       -
//    rewritten
//  VALU writes SGPR -> VMEM reads it (address/      5     none: the store/load bases s[64:71]   -
//    soffset)                                              are SALU-written
//  s_set_gpr_idx_on -> indexed VALU, _off -> plain   0     DECIDE16R / DECIDE16C / COMMIT16 /   (the indexed moves sit between
//                                                          INSERT16R (none is open in a        on and off; no non-indexed VALU
//                                                          release scan or its tail); W16C's   read inside a region; DECIDE16C's
//                                                          surplus insert (MCS_FC_BMOVE_OOL)   v_cndmask is VOP3: the index goes
//                                                                                              to its VGPR operands, SRC0, SRC1
//                                                                                              and DST, its mask is an SGPR pair)
//  SALU writes M0 -> s_movrels / s_movreld         1     W16C's surplus insert at a batch end   s_nop 0 between; s_movreld follows
//    reads it                                              (FREE[r], m0 = 2r)                  with m0 untouched
//  s_set_gpr_idx_on overwrites M0                  -     DECIDE16C; W16C's surplus insert     m0 = the cursor is set after the
//                                                                                              decision's region, as in every
//                                                                                              form; the surplus insert's relative
//                                                                                              moves come before its region
//  VALU writes SGPR -> SALU reads it               0     W16C's row and LIVE compares (vcc   (interlocked)
//                                                          -> s_mov exec / s_bcnt1 / s_or), the
//                                                          record read's s45 -> s_cmp, the bulk
//                                                          move's masks (s[60:61] -> s_bcnt1,
//                                                          s_and exec)
//  VALU writes SGPR -> VALU reads it as a constant  0     the bulk move: v_cmp s[60:61] ->     (interlocked; not a lane select)
//                                                          v_mbcnt / v_cndmask; W16C's starts
//                                                          (MCS_FA_STARTS16C: v_cmp vcc, one
//                                                          v_sub, v_cndmask with vcc)
//  LDS instruction issued -> its address / data      0     the bulk move: v120 is formed again  (not in the ISA's table of required
//    VGPRs rewritten                                       right after each ds_read_b128        wait states, whose one row of this
//                                                          (its address only: a read has no     kind is the VMEM store above; beyond
//                                                          data VGPRs to be read later; the     that it rests on the GPU parity runs
//                                                          reads land in the rows' own quads,   of tests/test_gpu_deferred_insert.py's
//                                                          which nothing touches before the     bulk-move cases, which differ per
//                                                          one s_waitcnt lgkmcnt(0) behind them) entry in finish, request and node)
//  s_setpc_b64 to a computed address               -     W16C's MCS_FC_RET / MCS_FC_RETW      the table of branches starts on a
//                                                                                              512-byte line and is 320 bytes, so
//                                                                                              s74 + 32 * entry + 4 * (t & 7), with
//                                                                                              32 * s43 (s43 <= 2) more, never
//                                                                                              carries into s59
// A reorder that moves a consumer next to its producer in the table must add the s_nop.

// progress-based wave priority at each batch end: the fewer of its jobs a wave has decided, the higher
// its issue priority (s_setprio 3 while more than J/2 of the wave's jobs remain, 2 while more than J/4,
// 1 while more than J/8, else 0).  The waves sharing a SIMD then keep pace, instead of the oldest racing
// ahead under age-ordered issue and the youngest finishing alone, latency-bound, after the others have
// left.  r04 A/B (profiles/r04_prio_*, r04_geo*): quarters of J against no priority, C4 FIFO 8.08 ->
// 7.25 ms, C4 DELAY 7.58 -> 6.80, Level1-heavy DELAY 29.6 -> 26.3; these halving thresholds, which
// tighten the pack towards the end, a further 7.28 -> 7.08 and 26.45 -> 26.02 (1/4, 1/8, 1/16 lost;
// 1/2, 1/4, 1/16 tied).  s76 scratch (SCC from the subtraction: 0 remaining once the cursor passed J);
// P prefixes the labels.
#define MCS_FA_PRIO(P)                                                                            \
    "s_sub_u32 s76, s42, s57\n\t"                                                                 \
    "s_cselect_b32 s76, 0, s76\n\t"                                                               \
    "s_lshl_b32 s76, s76, 1\n\t"                                                                  \
    "s_cmp_gt_u32 s76, s42\n\t"                                                                   \
    "s_cbranch_scc0 " P "p2_%=\n\t"                                                              \
    "s_setprio 3\n\t"                                                                            \
    "s_branch " P "pe_%=\n"                                                                       \
    P "p2_%=:\n\t"                                                                               \
    "s_lshl_b32 s76, s76, 1\n\t"                                                                  \
    "s_cmp_gt_u32 s76, s42\n\t"                                                                   \
    "s_cbranch_scc0 " P "p1_%=\n\t"                                                              \
    "s_setprio 2\n\t"                                                                            \
    "s_branch " P "pe_%=\n"                                                                       \
    P "p1_%=:\n\t"                                                                               \
    "s_lshl_b32 s76, s76, 1\n\t"                                                                  \
    "s_cmp_gt_u32 s76, s42\n\t"                                                                   \
    "s_cbranch_scc0 " P "p0_%=\n\t"                                                              \
    "s_setprio 1\n\t"                                                                            \
    "s_branch " P "pe_%=\n"                                                                       \
    P "p0_%=:\n\t"                                                                               \
    "s_setprio 0\n"                                                                               \
    P "pe_%=:\n\t"

// Register map of the loop (all fixed; listed as clobbers).
//   s40 t     s41 min(64, J - cb)  s42 J   s43 have_w  s44 flags  s45 arr   s46 dur
//   s47 cursor's lane in the batch (r - cb)  s48 (W16: {cores|mem<<16}) / s[48:49] cores, mem
//   (W16 forms: s49 = 0x100;  fused: s59 its own, see there)
//   s50 fl   s51 byte mask of fl   s52 8 * chunk   s53 register index of the chunk
//   s[54:55] kx, finish   s56 next clock   s57 cb   s[60:61] lanes with a free row
//   s[62:63] one-lane exec masks   s[64:65] jobs  s[66:67] out_node  s[68:69] out_start
//   s[70:71] out_finish  s72/s73 perm selectors   s74 t + 1  s75 expired  s76 tmp
//   s77 the wave's earliest finish  s78/s79 failed fits / bound 4J + 256 (a runaway loop ends as a
//   pool overflow: the engine re-runs the cluster on the compiled kernel)   s80 used  s81 peak
//   s82 waited
//   s83 passes without a decision  s84 release scans  s85 insert lane
//   release: row expiry masks in s[50:55], s[60:63], s[86:91]
//   v[64:71] nodes (W32: pairs {C, M} per chunk; W16: v64-v67)   v[72:79] fit-test differences
//   v80-v86 fit bits / byte mask   (release: finish rows in v[72:87])
//   v89 free rows  v90 earliest finish  v91-92 result batch (kx, start; finish = start + dur at
//   the store)
//   v[94:97] records  v[98:101] next records   v107 slot column  v108 node column  v109 node base
//   v110 lane  v111 -1   v[112:113] payload  v[114:115] {node address, fin}  v117 slot address
//   v118 frm - 1  v120 DPP min / scan temp  v121 address  v[122:123] payload  v124 lane minimum
//   v125-v127 store temps
// (W16C, the streamed W16R loop: s49, s[58:59], s74, s77-s79, s82 and s[86:101] have their own
// meaning, v87 holds a column, v106 the LIVE column, v89 nothing, its slot rows are the quads v[32:63], v92
// holds no start for a live lane, s75 is the bulk move's: see "W16C" below)
#define MCS_FA_CLOBBERS                                                                            \
    "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53",  \
        "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66",     \
        "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77", "s78", "s79",     \
        "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "v32",     \
        "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45",     \
        "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v64",                   \
        "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77",     \
        "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v89", "v90", "v91",     \
        "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v107", "v108",        \
        "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v117", "v118", "v119", "v120",        \
        "v121", "v122", "v123", "v124", "v125", "v126", "v127", "vcc", "scc", "m0", "exec", "memory"     \
        MCS_FA_STAMP_CLOBBERS

// the fused loop's clobbers: MCS_FA_CLOBBERS less the state it keeps in register-bound operands
// (MCS_FA_LOOP_F: s40 s43 s44 s47 s57 s59 s77 s78 s80-s84, v32-v55, v64-v67, v89-v93, v98-v101)
#define MCS_FF_CLOBBERS \
    "s41", "s42", "s45", "s46", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55", "s56", \
        "s58", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", \
        "s71", "s72", "s73", "s74", "s75", "s76", "s79", "s85", "s86", "s87", "s88", "s89", \
        "s90", "s91", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", \
        "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v94", "v95", \
        "v96", "v97", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", \
        "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", \
        "vcc", "scc", "m0", "exec", "memory" \
        MCS_FA_STAMP_CLOBBERS

// ---- W-specific pieces ----------------------------------------------------------------------
// the insert's candidate lanes: the lanes with a free slot row (computed early, off the chain)
#define MCS_FA_FREELANES "v_cmp_ne_u32_e64 s[60:61], 0, v89\n\t"
#define MCS_FA_FREELANES32 MCS_FA_FREELANES
#define MCS_FA_FREELANES16 ""
#define MCS_FA_FREELANES16R ""

// first fit (scheduler.go:129-137): byte c of v86 is 0xff where chunk c of the lane fits
#define MCS_FA_FIT32                                                                              \
    "v_subrev_u32 v72, s48, v64\n\t"                                                              \
    "v_subrev_u32 v73, s49, v65\n\t"                                                              \
    "v_subrev_u32 v74, s48, v66\n\t"                                                              \
    "v_subrev_u32 v75, s49, v67\n\t"                                                              \
    "v_subrev_u32 v76, s48, v68\n\t"                                                              \
    "v_subrev_u32 v77, s49, v69\n\t"                                                              \
    "v_subrev_u32 v78, s48, v70\n\t"                                                              \
    "v_subrev_u32 v79, s49, v71\n\t"                                                              \
    "v_and_b32 v80, v72, v73\n\t"                                                                 \
    "v_and_b32 v81, v74, v75\n\t"                                                                 \
    "v_and_b32 v82, v76, v77\n\t"                                                                 \
    "v_and_b32 v83, v78, v79\n\t"                                                                 \
    "v_perm_b32 v84, v81, v80, s72\n\t" /* bytes 0/1 = 0xff if chunk 0/1 fits */                  \
    "v_perm_b32 v85, v83, v82, s73\n\t" /* bytes 2/3 for chunks 2/3 */                            \
    "v_or_b32 v86, v84, v85\n\t"
#define MCS_FA_FIT16                                                                              \
    "v_pk_sub_u16 v72, v64, s48\n\t"                                                              \
    "v_pk_sub_u16 v73, v65, s48\n\t"                                                              \
    "v_pk_sub_u16 v74, v66, s48\n\t"                                                              \
    "v_pk_sub_u16 v75, v67, s48\n\t"                                                              \
    "v_and_b32_sdwa v80, v72, v72 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_0\n\t" \
    "v_and_b32_sdwa v81, v74, v74 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_0\n\t" \
    "v_and_b32_sdwa v80, v73, v73 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:WORD_0\n\t" \
    "v_and_b32_sdwa v81, v75, v75 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:WORD_0\n\t" \
    /* a VALU that reads a register right after an SDWA write preserving its other word sees  */  \
    /* the old word (measured: chunk 3 never fitted): the insert's free-row lanes and rows go */  \
    /* between the last SDWA write and the v_perm */                                              \
    "v_cmp_lt_u32_e64 s[60:61], s49, v89\n\t" /* (v89 = free rows | 0x100, s49 = 0x100) */      \
    "v_ffbl_b32 v117, v89\n\t" /* lowest free row; 8 (the sentinel) when none */               \
    "v_perm_b32 v86, v81, v80, s72\n\t" /* byte c = sign of chunk c's bit 15 / 31 */

// register index of the chunk (s52 = 8 * chunk) and the commit (cluster.go:146-147)
#define MCS_FA_COMMIT32                                                                           \
    "s_lshr_b32 s53, s52, 2\n\t"                                                                  \
    "s_lshl3_add_u32 s54, s52, s50\n\t" /* kx = chunk * 64 + fl */                                \
    "s_add_u32 s55, s40, s46\n\t"       /* finish */                                              \
    "s_set_gpr_idx_on s53, gpr_idx(SRC0,DST)\n\t"                                                 \
    "v_mov_b32 v64, v72\n\t"                                                                      \
    "v_mov_b32 v65, v73\n\t"                                                                      \
    "s_set_gpr_idx_off\n\t"
#define MCS_FA_COMMIT16                                                                           \
    "s_lshr_b32 s53, s52, 3\n\t"                                                                  \
    "s_lshl3_add_u32 s54, s52, s50\n\t"                                                           \
    "s_set_gpr_idx_on s53, gpr_idx(SRC0,DST)\n\t"                                                 \
    "v_mov_b32 v64, v72\n\t"                                                                      \
    "s_set_gpr_idx_off\n\t"

// slot insert (exec = the insert lane): payload, {node address, finish}, the LDS node commit
#define MCS_FA_INSERT32                                                                           \
    "v_mov_b64 v[112:113], s[48:49]\n\t"                                                          \
    "v_lshl_add_u32 v114, s54, 3, v109\n\t"                                                       \
    "v_mov_b32 v115, s55\n\t"                                                                     \
    "v_ffbl_b32 v117, v89\n\t"                                                                    \
    "v_lshl_add_u32 v117, v117, 9, v107\n\t"                                                      \
    "v_add_u32 v118, -1, v89\n\t"                                                                 \
    "ds_sub_u64 v114, v[112:113]\n\t"                                                             \
    "ds_write_b64 v117, v[112:113]\n\t"                                                           \
    "ds_write_b64 v117, v[114:115] offset:4096\n\t"                                               \
    "v_and_b32 v89, v118, v89\n\t"
#define MCS_FA_INSERT16                                                                           \
    "v_mov_b32 v112, s48\n\t"                                                                     \
    "v_lshl_add_u32 v114, s54, 2, v109\n\t"                                                       \
    "v_mov_b32 v115, s55\n\t"                                                                     \
    "v_lshl_add_u32 v117, v117, 9, v107\n\t" /* (v117 = the lane's lowest free row, FIT16) */    \
    "v_add_u32 v118, -1, v89\n\t"                                                                 \
    "ds_sub_u32 v114, v112\n\t"                                                                   \
    "ds_write_b32 v117, v112\n\t"                                                                 \
    "ds_write_b64 v117, v[114:115] offset:4096\n\t"                                               \
    "v_and_b32 v89, v118, v89\n\t"

// the record at the cursor (s47) to the scalar unit
#define MCS_FA_REC32                                                                              \
    "v_readlane_b32 s45, v94, s47\n\t"                                                            \
    "v_readlane_b32 s46, v95, s47\n\t"                                                            \
    "v_readlane_b32 s48, v96, s47\n\t"                                                            \
    "v_readlane_b32 s49, v97, s47\n\t"
#define MCS_FA_REC16                                                                              \
    "v_readlane_b32 s45, v94, s47\n\t"                                                            \
    "v_readlane_b32 s46, v95, s47\n\t"                                                            \
    "v_readlane_b32 s48, v96, s47\n\t"

// one release row p (cluster.go:153-157): expiry lane mask MASK, node address NODE
#define MCS_FA_ROW(W, p, NODE, MASK)                                                              \
    "s_cmp_lg_u64 " MASK ", 0\n\t"                                                                \
    "s_cbranch_scc0 mcsfa_r" #p "_%=\n\t"                                                         \
    "s_bcnt1_i32_b64 s76, " MASK "\n\t"                                                           \
    "s_mov_b64 exec, " MASK "\n\t" MCS_FA_PAYREAD##W(p) "s_add_u32 s75, s75, s76\n\t"            \
    "s_waitcnt lgkmcnt(0)\n\t" MCS_FA_PAYADD##W(NODE)                                             \
    "ds_write_b32 v107, v111 offset:4096+" #p "*512+4\n\t"                                        \
    "v_or_b32 v89, 1<<" #p ", v89\n\t"                                                            \
    "s_mov_b64 exec, -1\n"                                                                        \
    "mcsfa_r" #p "_%=:\n\t"
#define MCS_FA_PAYREAD32(p) "ds_read_b64 v[122:123], v107 offset:" #p "*512\n\t"
#define MCS_FA_PAYREAD16(p) "ds_read_b32 v122, v107 offset:" #p "*512\n\t"
#define MCS_FA_PAYADD32(NODE) "ds_add_u64 " NODE ", v[122:123]\n\t"
#define MCS_FA_PAYADD16(NODE) "ds_add_u32 " NODE ", v122\n\t"

#define MCS_FA_RELEASE(W)                                                                         \
    "ds_read_b64 v[72:73], v107 offset:4096+0*512\n\t"                                            \
    "ds_read_b64 v[74:75], v107 offset:4096+1*512\n\t"                                            \
    "ds_read_b64 v[76:77], v107 offset:4096+2*512\n\t"                                            \
    "ds_read_b64 v[78:79], v107 offset:4096+3*512\n\t"                                            \
    "ds_read_b64 v[80:81], v107 offset:4096+4*512\n\t"                                            \
    "ds_read_b64 v[82:83], v107 offset:4096+5*512\n\t"                                            \
    "ds_read_b64 v[84:85], v107 offset:4096+6*512\n\t"                                            \
    "ds_read_b64 v[86:87], v107 offset:4096+7*512\n\t"                                            \
    "s_not_b32 s76, s74\n\t"                                                                      \
    "v_mov_b32 v124, s76\n\t"                                                                     \
    "s_mov_b32 s75, 0\n\t"                                                                        \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                    \
    "v_cmp_ge_u32_e64 s[50:51], s40, v73\n\t"                                                     \
    "v_cmp_ge_u32_e64 s[52:53], s40, v75\n\t"                                                     \
    "v_cmp_ge_u32_e64 s[54:55], s40, v77\n\t"                                                     \
    "v_cmp_ge_u32_e64 s[60:61], s40, v79\n\t"                                                     \
    "v_cmp_ge_u32_e64 s[62:63], s40, v81\n\t"                                                     \
    "v_cmp_ge_u32_e64 s[86:87], s40, v83\n\t"                                                     \
    "v_cmp_ge_u32_e64 s[88:89], s40, v85\n\t"                                                     \
    "v_cmp_ge_u32_e64 s[90:91], s40, v87\n\t"                                                     \
    /* earliest remaining finish: d = finish - (t + 1) wraps for expired rows */                  \
    "v_subrev_u32 v73, s74, v73\n\t"                                                              \
    "v_subrev_u32 v75, s74, v75\n\t"                                                              \
    "v_subrev_u32 v77, s74, v77\n\t"                                                              \
    "v_subrev_u32 v79, s74, v79\n\t"                                                              \
    "v_subrev_u32 v81, s74, v81\n\t"                                                              \
    "v_subrev_u32 v83, s74, v83\n\t"                                                              \
    "v_subrev_u32 v85, s74, v85\n\t"                                                              \
    "v_subrev_u32 v87, s74, v87\n\t"                                                              \
    "v_min3_u32 v124, v124, v73, v75\n\t"                                                         \
    "v_min3_u32 v120, v77, v79, v81\n\t"                                                          \
    "v_min3_u32 v124, v124, v83, v85\n\t"                                                         \
    "v_min3_u32 v124, v124, v87, v120\n\t"                                                        \
    MCS_FA_ROW(W, 0, "v72", "s[50:51]") MCS_FA_ROW(W, 1, "v74", "s[52:53]")                       \
    MCS_FA_ROW(W, 2, "v76", "s[54:55]") MCS_FA_ROW(W, 3, "v78", "s[60:61]")                       \
    MCS_FA_ROW(W, 4, "v80", "s[62:63]") MCS_FA_ROW(W, 5, "v82", "s[86:87]")                       \
    MCS_FA_ROW(W, 6, "v84", "s[88:89]") MCS_FA_ROW(W, 7, "v86", "s[90:91]")                       \
    "s_sub_u32 s80, s80, s75\n\t"

// the whole clock-advance release: rows, node reload issued, earliest remaining finish in v90
#define MCS_FA_SCAN32 MCS_FA_RELEASE(32) MCS_FA_RELOAD32 "v_add_u32 v90, s74, v124\n\t"
#define MCS_FA_SCAN16 MCS_FA_RELEASE(16) MCS_FA_RELOAD16 "v_add_u32 v90, s74, v124\n\t"

// ---- W16R: the 16-bit node format with the running slots in registers ----------------------------
// Slot row r of a lane is v(32+r) finish, v(40+r) payload {cores | mem << 16}, v(48+r) the node's
// LDS address: an insert is three indexed moves (row from v_ffbl of the insert lane's free rows,
// broadcast with one v_readlane), and a release reads no slot from LDS — its only round trip is
// the node reload, issued before the earliest-finish minimum that hides it.
#define MCS_FA_FIT16R MCS_FA_FIT16
#define MCS_FA_COMMIT16R MCS_FA_COMMIT16
#define MCS_FA_REC16R MCS_FA_REC16
#define MCS_FA_TAKE16R MCS_FA_TAKE16
#define MCS_FA_RELOAD16R MCS_FA_RELOAD16
#define MCS_FA_INIT32 ""
#define MCS_FA_INIT16 "s_mov_b32 s49, 0x100\n\t"
#define MCS_FA_INIT16R                                                                            \
    "s_mov_b32 s49, 0x100\n\t"                                                                   \
    "v_mov_b32 v32, -1\n\t"                                                                      \
    "v_mov_b32 v33, -1\n\t"                                                                      \
    "v_mov_b32 v34, -1\n\t"                                                                      \
    "v_mov_b32 v35, -1\n\t"                                                                      \
    "v_mov_b32 v36, -1\n\t"                                                                      \
    "v_mov_b32 v37, -1\n\t"                                                                      \
    "v_mov_b32 v38, -1\n\t"                                                                      \
    "v_mov_b32 v39, -1\n\t"
// (exec = the insert lane, or empty when the pool is full; s73 = the node array's LDS base)
#define MCS_FA_INSERT16R                                                                          \
    "v_readlane_b32 s86, v117, s85\n\t" /* 0-7, or 8 with exec empty: in range either way */   \
    "s_lshl2_add_u32 s87, s54, s73\n\t"                                                          \
    "s_lshl_b32 s76, 1, s86\n\t"                                                                 \
    "s_set_gpr_idx_on s86, gpr_idx(DST)\n\t"                                                     \
    "v_mov_b32 v32, s55\n\t"                                                                     \
    "v_mov_b32 v40, s48\n\t"                                                                     \
    "v_mov_b32 v48, s87\n\t"                                                                     \
    "s_set_gpr_idx_off\n\t"                                                                      \
    "v_xor_b32 v89, s76, v89\n\t" /* the row is taken */
// (exec = the row's expiry mask, SCC = any: no separate test, and exec is restored to the full
// wave once after the last row).  r05: a row with an expiry branches to its body out of line
// (MCS_FR_BODY, placed by the loop after an unconditional branch) and returns; a row without one
// falls through.  ~1.5 of the 8 rows expire per scan, so a scan takes ~3 taken branches instead of
// ~6.5: at one wave per SIMD a taken branch costs ~20 cycles, the row test ~8.
#define MCS_FR_ROW(p, MASK, F, P, A)                                                              \
    "s_and_b64 exec, " MASK ", -1\n\t"                                                           \
    "s_cbranch_scc1 mcsfa_rb" #p "_%=\n"                                                         \
    "mcsfa_r" #p "_%=:\n\t"
// (a row's release under exec = its expiry mask: the payloads back to the nodes, the slots free, counted)
#define MCS_FR_REL(p, MASK, F, P, A)                                                              \
    "s_bcnt1_i32_b64 s76, " MASK "\n\t"                                                          \
    "ds_add_u32 " A ", " P "\n\t"                                                               \
    "v_mov_b32 " F ", -1\n\t"                                                                    \
    "s_add_u32 s75, s75, s76\n\t"                                                                \
    "v_or_b32 v89, 1<<" #p ", v89\n\t"
#define MCS_FR_BODY(p, MASK, F, P, A)                                                             \
    "mcsfa_rb" #p "_%=:\n\t" MCS_FR_REL(p, MASK, F, P, A)                                        \
    "s_branch mcsfa_r" #p "_%=\n"
#define MCS_FA_SCAN16R                                                                            \
    /* the LDS node copy is refreshed from the registers first (commits do not touch it) */       \
    "ds_write_b32 v108, v64 offset:0\n\t"                                                        \
    "ds_write_b32 v108, v65 offset:256\n\t"                                                      \
    "ds_write_b32 v108, v66 offset:512\n\t"                                                      \
    "ds_write_b32 v108, v67 offset:768\n\t"                                                      \
    "s_mov_b32 s75, 0\n\t"                                                                       \
    "v_cmp_ge_u32_e64 s[50:51], s40, v32\n\t"                                                    \
    "v_cmp_ge_u32_e64 s[52:53], s40, v33\n\t"                                                    \
    "v_cmp_ge_u32_e64 s[54:55], s40, v34\n\t"                                                    \
    "v_cmp_ge_u32_e64 s[60:61], s40, v35\n\t"                                                    \
    "v_cmp_ge_u32_e64 s[62:63], s40, v36\n\t"                                                    \
    "v_cmp_ge_u32_e64 s[86:87], s40, v37\n\t"                                                    \
    "v_cmp_ge_u32_e64 s[88:89], s40, v38\n\t"                                                    \
    "v_cmp_ge_u32_e64 s[90:91], s40, v39\n\t"                                                    \
    MCS_FR_ROW(0, "s[50:51]", "v32", "v40", "v48") MCS_FR_ROW(1, "s[52:53]", "v33", "v41", "v49")  \
    MCS_FR_ROW(2, "s[54:55]", "v34", "v42", "v50") MCS_FR_ROW(3, "s[60:61]", "v35", "v43", "v51")  \
    MCS_FR_ROW(4, "s[62:63]", "v36", "v44", "v52") MCS_FR_ROW(5, "s[86:87]", "v37", "v45", "v53")  \
    MCS_FR_ROW(6, "s[88:89]", "v38", "v46", "v54") MCS_FR_ROW(7, "s[90:91]", "v39", "v47", "v55")  \
    "s_mov_b64 exec, -1\n\t"                                                                     \
    "s_sub_u32 s80, s80, s75\n\t" MCS_FA_RELOAD16                                               \
    /* the lane's earliest remaining finish (released rows now hold -1) */                     \
    "v_min3_u32 v90, v32, v33, v34\n\t"                                                          \
    "v_min3_u32 v90, v90, v35, v36\n\t"                                                          \
    "v_min3_u32 v90, v90, v37, v38\n\t"                                                          \
    "v_min_u32 v90, v90, v39\n\t"
// the expiring rows' bodies of MCS_FA_SCAN16R (out of line: after an unconditional branch)
#define MCS_FA_RBODY16R                                                                           \
    MCS_FR_BODY(0, "s[50:51]", "v32", "v40", "v48") MCS_FR_BODY(1, "s[52:53]", "v33", "v41", "v49") \
    MCS_FR_BODY(2, "s[54:55]", "v34", "v42", "v50") MCS_FR_BODY(3, "s[60:61]", "v35", "v43", "v51") \
    MCS_FR_BODY(4, "s[62:63]", "v36", "v44", "v52") MCS_FR_BODY(5, "s[86:87]", "v37", "v45", "v53") \
    MCS_FR_BODY(6, "s[88:89]", "v38", "v46", "v54") MCS_FR_BODY(7, "s[90:91]", "v39", "v47", "v55")
#define MCS_FA_RBODY16S                                                                           \
    MCS_FR_BODY(0, "s[50:51]", "v32", "v40", "v48") MCS_FR_BODY(1, "s[52:53]", "v33", "v41", "v49")
#define MCS_FA_RBODY32 ""
#define MCS_FA_RBODY16 ""

// node registers back from the LDS copy
#define MCS_FA_RELOAD32                                                                           \
    "ds_read_b64 v[64:65], v108 offset:0\n\t"                                                     \
    "ds_read_b64 v[66:67], v108 offset:512\n\t"                                                   \
    "ds_read_b64 v[68:69], v108 offset:1024\n\t"                                                  \
    "ds_read_b64 v[70:71], v108 offset:1536\n\t"
#define MCS_FA_RELOAD16                                                                           \
    "ds_read_b32 v64, v108 offset:0\n\t"                                                          \
    "ds_read_b32 v65, v108 offset:256\n\t"                                                        \
    "ds_read_b32 v66, v108 offset:512\n\t"                                                        \
    "ds_read_b32 v67, v108 offset:768\n\t"

// the next batch's records (prefetched in v[98:101]) become current, requests clamped
#define MCS_FA_TAKE32                                                                             \
    "v_mov_b32 v94, v98\n\t"                                                                      \
    "v_mov_b32 v95, v99\n\t"                                                                      \
    "v_min_u32 v96, 0x7fffffff, v100\n\t"                                                         \
    "v_min_u32 v97, 0x7fffffff, v101\n\t"
#define MCS_FA_TAKE16                                                                             \
    "v_mov_b32 v94, v98\n\t"                                                                      \
    "v_mov_b32 v95, v99\n\t"                                                                      \
    "v_min_u32 v96, 0x7fff, v100\n\t"                                                             \
    "v_min_u32 v97, 0x7fff, v101\n\t"                                                             \
    "v_lshl_or_b32 v96, v97, 16, v96\n\t"

// ---- per-form hooks of the loop -----------------------------------------------------------------
// a decided placement: the fitting lane's chunk, the commit under exec = that lane, then the
// running-slot insert under exec = the lowest lane with a free row (none: exec empty)
#define MCS_FA_DECIDE_(W)                                                                         \
    MCS_FA_PICK1##W MCS_FA_FREELANES##W                                                           \
    "s_lshl_b64 exec, 1, s50\n\t" MCS_FA_PICK2##W MCS_FA_COMMIT##W                                \
    "s_ff1_i32_b64 s85, s[60:61]\n\t"                                                             \
    "s_lshl_b64 s[62:63], 1, s85\n\t"                                                             \
    "s_and_b64 exec, s[62:63], s[60:61]\n\t" MCS_FA_INSERT##W
#define MCS_FA_DECIDE32 MCS_FA_DECIDE_(32)
#define MCS_FA_DECIDE16 MCS_FA_DECIDE_(16)
#define MCS_FA_DECIDE16S MCS_FA_DECIDE_(16S)
// W16R: ONE register-index region for both moves (the commit's chunk, then the insert's row by
// s_set_gpr_idx_idx); the insert lane and its row are found before it (VALU reads inside the
// region would be indexed), the row is taken after it
#define MCS_FA_DECIDE16R                                                                          \
    "v_readlane_b32 s51, v86, s50\n\t"                                                            \
    "s_ff1_i32_b64 s85, s[60:61]\n\t"                                                             \
    "s_lshl_b64 exec, 1, s50\n\t"                                                                 \
    "v_readlane_b32 s86, v117, s85\n\t" /* 0-7, or 8 with exec empty: in range either way */    \
    "s_ff1_i32_b32 s52, s51\n\t"                                                                  \
    "s_lshr_b32 s53, s52, 3\n\t"                                                                  \
    "s_lshl3_add_u32 s54, s52, s50\n\t"                                                           \
    "s_set_gpr_idx_on s53, gpr_idx(SRC0,DST)\n\t"                                                 \
    "v_mov_b32 v64, v72\n\t" /* the commit (cluster.go:146-147) */                                \
    "s_lshl_b64 s[62:63], 1, s85\n\t"                                                             \
    "s_and_b64 exec, s[62:63], s[60:61]\n\t"                                                      \
    "s_lshl2_add_u32 s87, s54, s73\n\t"                                                           \
    "s_set_gpr_idx_idx s86\n\t"                                                                   \
    "v_mov_b32 v32, s55\n\t" /* the slot: finish, payload, node address (SGPR sources) */        \
    "v_mov_b32 v40, s48\n\t"                                                                      \
    "v_mov_b32 v48, s87\n\t"                                                                      \
    "s_set_gpr_idx_off\n\t"                                                                       \
    "s_lshl_b32 s76, 1, s86\n\t"                                                                  \
    "v_xor_b32 v89, s76, v89\n\t" /* the row is taken */
// lanes with a fit into vcc
#define MCS_FA_ANYFIT "v_cmp_ne_u32_e32 vcc, 0, v86\n\t"
#define MCS_FA_ANYFIT32 MCS_FA_ANYFIT
#define MCS_FA_ANYFIT16 MCS_FA_ANYFIT
#define MCS_FA_ANYFIT16R MCS_FA_ANYFIT
// the fitting lane's byte mask (PICK1, a broadcast) and its lowest fitting chunk (PICK2)
#define MCS_FA_PICK1 "v_readlane_b32 s51, v86, s50\n\t"
#define MCS_FA_PICK2 "s_ff1_i32_b32 s52, s51\n\t" /* 8 * the lane's first fitting chunk */
#define MCS_FA_PICK132 MCS_FA_PICK1
#define MCS_FA_PICK116 MCS_FA_PICK1
#define MCS_FA_PICK116R MCS_FA_PICK1
#define MCS_FA_PICK232 MCS_FA_PICK2
#define MCS_FA_PICK216 MCS_FA_PICK2
#define MCS_FA_PICK216R MCS_FA_PICK2
// a zero-duration job's node (kx into s54; m0 = the cursor for the result writes)
#define MCS_FA_ZEROKX                                                                             \
    "v_readlane_b32 s51, v86, s50\n\t"                                                           \
    "s_mov_b32 m0, s47\n\t"                                                                      \
    "s_ff1_i32_b32 s52, s51\n\t"                                                                 \
    "s_lshl3_add_u32 s54, s52, s50\n\t"
#define MCS_FA_ZEROKX32 MCS_FA_ZEROKX
#define MCS_FA_ZEROKX16 MCS_FA_ZEROKX
#define MCS_FA_ZEROKX16R MCS_FA_ZEROKX
// What the streamed entry and exit (MCS_FA_ENTRY_S / MCS_FA_EXIT_S) take per form, W16C's with its
// macros below: the runaway guard's start (the shared pass counts the failed fits up in s78 against the
// bound 4J + 256 in s79), where the loop's head lies right after the entry (W16C places it; nothing falls
// into it but the entry, once), and the WaitQueue statistic at the exit.
#define MCS_FA_GUARD0_                                                                            \
    "s_mov_b32 s78, 0\n\t"                                                                        \
    "s_lshl2_add_u32 s79, s42, 0x100\n\t"
#define MCS_FA_GUARD032 MCS_FA_GUARD0_
#define MCS_FA_GUARD016 MCS_FA_GUARD0_
#define MCS_FA_GUARD016S MCS_FA_GUARD0_
#define MCS_FA_HEAD32 ""
#define MCS_FA_HEAD16 ""
#define MCS_FA_HEAD16S ""
#define MCS_FA_XWAITED_ "s_mov_b32 %[waited], s82\n\t"
#define MCS_FA_XWAITED32 MCS_FA_XWAITED_
#define MCS_FA_XWAITED16 MCS_FA_XWAITED_
#define MCS_FA_XWAITED16S MCS_FA_XWAITED_
// the result batch's start column (v92) before it is read, at the batch end's stores and at the exit:
// complete in every form that writes a start at the placement; W16C forms its live lanes' here
#define MCS_FA_STARTS32 ""
#define MCS_FA_STARTS16 ""
#define MCS_FA_STARTS16S ""
#define MCS_FA_STARTS16R ""
// slots of the pool (64 lanes x P rows)
#define MCS_FA_POOLMAX32 "64*8"
#define MCS_FA_POOLMAX16 "64*8"
#define MCS_FA_POOLMAX16R "64*8"
// the result batch's node index from kx = chunk * 64 + lane
#define MCS_FA_NODEIDX                                                                            \
    "v_and_b32 v126, 63, v91\n\t"                                                                \
    "v_lshrrev_b32 v127, 6, v91\n\t"                                                             \
    "v_lshl_add_u32 v126, v126, 2, v127\n\t" /* node = lane * 4 + chunk */
#define MCS_FA_NODEIDX32 MCS_FA_NODEIDX
#define MCS_FA_NODEIDX16 MCS_FA_NODEIDX
#define MCS_FA_NODEIDX16R MCS_FA_NODEIDX

// ---- W16C: W16R with calendar slot rows (the streamed loop of the 129-256 node shape; DESIGN.md §4
// "Calendar rows") ------------------------------------------------------------------------------------
// A slot lives in row finish & 7, so a clock advance to second t compares ONE row, v(32 + 4 * (t & 7)),
// and the wave's earliest finish is not kept at all (no lane-minimum tree, no DPP chain, no s_min per
// insert).  Invariant, after the clock has been handled at second t: no slot has finish <= t; every
// slot sits in row finish & 7 but the misplaced ones (their row was full: they took the next row with
// a free lane); XMIN (s77) <= the earliest finish of any misplaced slot, 0xffffffff when there is none.
// The free slots are scalar lane masks, one per row.  A placement takes no slot: the job stays in its
// batch lane, its finish in the LIVE column v106 (-1 in every lane without a running job of the current
// batch), its node in v91 and its request in v96 as the result batch and the records hold them anyway; its
// start is not written at all while it is live (finish - v95, MCS_FA_STARTS16C).
// Whatever compares a calendar row against t compares LIVE first (the copies' row blocks, the sleep chain,
// the full scan as a ninth row, the exact minimum); a lane that expires hands its request back out of line
// (MCS_FC_BREL).  At the batch end the live lanes go into their rows together (MCS_FC_BMOVE), so the
// invariant above holds for the slots, and for LIVE: no lane has finish <= t.  A batch-lane job is compared
// every second and is never misplaced: XMIN knows nothing of it.
//   s[86:101] FREE[0..7]: the free lanes of each row (row r: s[86+2r:87+2r]), static registers for a release
//             and the bulk move, s_movrels/s_movreld (m0 = 2r) for a surplus job's insert
//   s77 XMIN   s74, s59 the address of the copies' table of branches (MCS_FC_RET; on a 512-byte line),
//   low and high word   s[58:59] a computed jump's target   s49 a computed jump's t & 7 / the full scan's
//   released count / a batch-lane release's row count   s79 the limit of a waiting head's sleep,
//   min(XMIN, t + 9)   s[50:55], s[60:63], s75, s85: the decision's pick (s50-s54), its lane mask (s[60:61])
//   and the bulk move's temporaries   s43 1 while a head waits in
//   a copy's section, 2 while a zero-duration job waits out of line, else 0   s41 min(64, J - cb), read where a
//   batch is taken only   v89, v90, v107 the record columns shifted by one lane (MCS_FC_SHIFT)   m0 after a
//   placement: the lane of the job placed, the record read's lane select
//   s78 the failed fits left of the runaway bound   s82 the WaitQueue heads placed (a head waiting at
//   the exit is s43)   v87 the batch's true arrival column (v94 holds 0xffffffff for its zero-duration
//   jobs; both 0xffffffff in the lanes past the stream's end)   s75 is not used
// The clock moves in three ways.  By one second (the placed WaitQueue head; each step of a failed fit's
// sleep has a block of its own, MCS_FC_WSL) or to a second nothing can finish before (an arrival one
// second on): the XMIN test and the row block of the copy of that second (MCS_FC_COPY: the next copy's
// after a one-second advance, through mcsfa_adv1's computed jump otherwise), which compares the row
// and either leaves at once (mcsfa_norel: no LDS traffic) or releases it and falls into the tail
// (mcsfa_reltail: node reload, the head's fit test, and into the pass at mcsfa_fitted).  By more
// than a second (an arrival gap), or with a misplaced slot due (t >= XMIN): mcsfa_full, every row in
// turn against t, and after one that XMIN asked for, XMIN rebuilt as the minimum over the slots with
// finish & 7 != row (free slots hold -1 and drop out; a gap's full scan at t < XMIN releases no
// misplaced slot, so XMIN stands, and stays exact).  A failed fit steps second by second in its copy's
// waiting-head section (each step the row compare and one test against min(XMIN, t + 9): MCS_FC_COPY,
// MCS_FC_WSL); after eight steps without a release every row has been compared, and the clock jumps to the
// exact earliest finish (lane-minimum tree + DPP, as every other form's scan end).  Nothing running
// is s80 == 0 (the count of the slots and the live lanes).  A release scan is counted where something is
// released, from a row, from the batch lanes or from both (mcsfa_reltail, mcsfa_wreltail, mcsfa_zreltail).
// Hazards (table above): s_set_gpr_idx_on overwrites m0, so m0 = the cursor is set after the decision's
// region as in every form; the row and LIVE compares write vcc, which s_cbranch_vccz / vccnz and SALU read
// (interlocked); the DPP chains keep s_nop 1; the surplus insert of the bulk move keeps the per-job
// insert's distances (s_nop 0 between m0 and s_movrels, both relative moves before its region).
//
// The fit test ("Fit and commit"): the four differences as in MCS_FA_FIT16; then one v_perm per
// pair of chunks sign-replicates byte 1 and byte 3 of both differences, the guard bits (s72 = 0x0b090a08:
// {c0, c1 | m0, m1}, the cores guards in the low half, the memory guards in the high half, every byte 0x00 or
// 0xff), and one SDWA AND of high half & low half per pair writes half of v86: byte c is 0xff exactly when
// chunk c fits, as MCS_FA_FIT16's v_perm leaves it, in nine vector instructions for ten.  Hazard table, row 2:
// the second v_perm lies between the two SDWA writes of v86 (the second preserves, so reads, the half the
// first wrote), and GAP, a scalar instruction of the caller's (the pass's finish, s_add s55; the release
// tail's arrival test, s_cmp_le), between the preserving write and the v_cmp that reads v86.
#define MCS_FA_FITBITS16C(GAP)                                                                    \
    "v_pk_sub_u16 v72, v64, s48\n\t"                                                              \
    "v_pk_sub_u16 v73, v65, s48\n\t"                                                              \
    "v_pk_sub_u16 v74, v66, s48\n\t"                                                              \
    "v_pk_sub_u16 v75, v67, s48\n\t"                                                              \
    "v_perm_b32 v80, v73, v72, s72\n\t" /* {c0, c1 | m0, m1} */                                   \
    "v_and_b32_sdwa v86, v80, v80 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_0\n\t" \
    "v_perm_b32 v81, v75, v74, s72\n\t" /* {c2, c3 | m2, m3} */                                   \
    "v_and_b32_sdwa v86, v81, v81 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:WORD_0\n\t" \
    GAP
#define MCS_FA_FIT16C MCS_FA_FITBITS16C("s_add_u32 s55, s40, s46\n\t") /* finish */
// (the record broadcasts stay: one s_load_dwordx4 per job into an SGPR quad, a pass ahead, measured
// faster at 512 clusters and slower at 4096, where the scalar port pays 7 instructions for the three
// v_readlane: DESIGN.md §4 "pass trim", profiles/pass_trim/steps_flagged.patch)
#define MCS_FA_REC16C MCS_FA_REC16
// Zero-duration jobs (1 in 600 of the reference's streams) leave the common pass through the test
// it runs anyway: when a batch is taken, the arrival column v94 gets 0xffffffff in the lanes of
// zero-duration jobs (the true arrivals stay in v87), so the head's arrival test sends such a job to
// mcsfa_arrive, which tells it apart by that arrival and takes it out of line (MCS_FC_ZROUTE):
// the true arrival's test, the fit test, and then mcsfa_znofit (it waits out of line) or mcsfa_zero.
// The pass itself has no duration test.  (The clock never reaches
// 0xffffffff in this loop and no arrival is 0xffffffff: the host bounds last arrival + sum(dur + 1)
// below it, and streams without that bound run the compiled kernel.  A non-zero job carrying that
// arrival would still sleep to it as before.)
#define MCS_FA_ZMASK16C(SRC)                                                                      \
    "v_mov_b32 v87, " SRC "\n\t"                                                                  \
    "v_cmp_eq_u32_e32 vcc, 0, v95\n\t"                                                            \
    "v_cndmask_b32_e32 v94, " SRC ", v111, vcc\n\t" /* (v111 = -1) */
#define MCS_FA_TAKE16C                                                                            \
    "v_mov_b32 v95, v99\n\t"                                                                      \
    "v_min_u32 v96, 0x7fff, v100\n\t"                                                             \
    "v_min_u32 v97, 0x7fff, v101\n\t"                                                             \
    "v_lshl_or_b32 v96, v97, 16, v96\n\t" MCS_FA_ZMASK16C("v98")
// The record read after a placement takes the NEXT job's record from the lane of the job just placed
// (m0), out of copies of the three record columns shifted down by one lane: v89 arrival, v90 duration,
// v107 request.  The arrival column carries 0xffffffff in every lane without a job (s41 = min(64, J - cb)
// on, in the last batch), and lane 63 of its shifted copy holds 0xffffffff too: "no next job in this
// batch" reads as an arrival that never comes, so the pass ends on the arrival test alone and
// mcsfa_arrive's out-of-line route (MCS_FC_ZROUTE) tells a batch end from a zero-duration job.  Built
// once per batch (the v_mov of v89 / v90 / v107 are the two wait states the DPP read of v94 needs, the
// s_nop 1 kept anyway; lane 63 of a wave_shl has no source and keeps the destination's -1).
#define MCS_FC_SHIFT                                                                              \
    "v_cmp_le_u32_e32 vcc, s41, v110\n\t"                                                         \
    "v_cndmask_b32_e32 v94, v94, v111, vcc\n\t" /* (v111 = -1) */                                 \
    "v_mov_b32 v89, -1\n\t"                                                                       \
    "v_mov_b32 v90, 0\n\t"                                                                        \
    "v_mov_b32 v107, 0\n\t"                                                                       \
    "s_nop 1\n\t"                                                                                 \
    "v_mov_b32_dpp v89, v94 wave_shl:1 row_mask:0xf bank_mask:0xf\n\t"                            \
    "v_mov_b32_dpp v90, v95 wave_shl:1 row_mask:0xf bank_mask:0xf\n\t"                            \
    "v_mov_b32_dpp v107, v96 wave_shl:1 row_mask:0xf bank_mask:0xf\n\t"
// the next job's record from the lane of the job just placed (m0)
#define MCS_FC_RECNEXT                                                                            \
    "v_readlane_b32 s45, v89, m0\n\t"                                                             \
    "v_readlane_b32 s46, v90, m0\n\t"                                                             \
    "v_readlane_b32 s48, v107, m0\n\t"
// The LDS node copy of this form is one 16-byte word per lane, chunk c of lane l at base + 16 * l +
// 4 * c (v108 = base + 16 * lane, 16-byte aligned): a release refreshes it with one ds_write_b128 of
// v[64:67] and reloads it with one ds_read_b128.  The decision's kx (s54) is then the node index
// lane * 4 + chunk itself: the slot's node address is still base + 4 * kx, and the result batch is
// stored without a conversion (fa_finish: KXNODE).
#define MCS_FA_RELOAD16C "ds_read_b128 v[64:67], v108\n\t"
#define MCS_FA_ZEROKX16C                                                                          \
    "v_readlane_b32 s51, v86, s50\n\t"                                                           \
    "s_mov_b32 m0, s47\n\t"                                                                      \
    "s_ff1_i32_b32 s52, s51\n\t"                                                                 \
    "s_lshr_b32 s53, s52, 3\n\t"                                                                 \
    "s_lshl2_add_u32 s54, s50, s53\n\t"
#define MCS_FA_POOLMAX16C "64*8"
#define MCS_FA_NODEIDX16C "v_mov_b32 v126, v91\n\t"
// A running job of the current batch has no start in v92: LIVE holds its finish and v95 its duration, and
// the start is formed where the lane leaves LIVE (MCS_FC_BREL, the full scan's ninth row) or, for the
// lanes still live, where the result batch is read: before the batch end's stores and at the exit (no live
// lane there when the run stopped at the first job of a new batch: the bulk move has left -1 in LIVE, and
// v95 is the new batch's).  No wrap: finish = start + duration, which the host bounds below 2^32 - 1.
// Zero-duration jobs never enter LIVE, their start is written at the placement (mcsfa_zero).
#define MCS_FA_STARTS16C                                                                          \
    "v_cmp_ne_u32_e32 vcc, -1, v106\n\t"                                                          \
    "v_sub_u32 v120, v106, v95\n\t"                                                               \
    "v_cndmask_b32_e32 v92, v92, v120, vcc\n\t"
// The WaitQueue statistic of this form is counted where the WaitQueue head is placed (the waiting-head
// section of MCS_FC_COPY, mcsfa_zhead: once per waited job, where the shared loop pays a subtract and an
// add at every failed fit); a head still waiting when the loop leaves (deadlock, the runaway guard:
// s43 = 1, or 2 for a zero-duration job, on exactly those exits, 0 on every other) is added at the exit.
#define MCS_FA_XWAITED16C                                                                         \
    "s_cmp_lg_u32 s43, 0\n\t"                                                                     \
    "s_addc_u32 %[waited], s82, 0\n\t"
// The runaway guard counts s78 down from the bound 4J + 256 and the borrow is its test (the failed fit
// number 4J + 257 trips it, as the shared loop's s78 > s79); s79 has another use in this form.
#define MCS_FA_GUARD016C "s_lshl2_add_u32 s78, s42, 0x100\n\t"
// The entry needs no padding: it reaches the copy of its clock through the table of branches, and each
// copy places its own head 24 bytes into a 64-byte instruction line (MCS_FC_COPY; 16 bytes before the fit
// test lost 8), the position that
// measured best of the eight 4-byte positions for the single loop at 4096 and at 512 clusters (where the
// loop lies decided up to 1.8 % and 3.4 % of its time, profiles/pass_trim/ab_place_*.txt,
// profiles/calendar_rows/ab_place_*.txt and profiles/fit_commit/ab_place_*.txt).
#define MCS_FA_HEAD16C ""
#define MCS_FA_INIT16C MCS_FA_ZMASK16C("v94") /* (batch 0) */                                     \
    "s_min_u32 s41, s42, 64\n\t" MCS_FC_SHIFT                                                     \
    "s_mov_b64 s[86:87], -1\n\t"                                                                 \
    "s_mov_b64 s[88:89], -1\n\t"                                                                 \
    "s_mov_b64 s[90:91], -1\n\t"                                                                 \
    "s_mov_b64 s[92:93], -1\n\t"                                                                 \
    "s_mov_b64 s[94:95], -1\n\t"                                                                 \
    "s_mov_b64 s[96:97], -1\n\t"                                                                 \
    "s_mov_b64 s[98:99], -1\n\t"                                                                 \
    "s_mov_b64 s[100:101], -1\n\t"                                                               \
    "s_getpc_b64 s[58:59]\n"                                                                      \
    "mcsfa_pc_%=:\n\t"                                                                            \
    "s_add_u32 s74, s58, mcsfa_tbl_%=-mcsfa_pc_%=\n\t"                                           \
    "s_addc_u32 s59, s59, 0\n\t"                                                                      \
    "v_mov_b32 v32, -1\n\t"                                                                      \
    "v_mov_b32 v36, -1\n\t"                                                                      \
    "v_mov_b32 v40, -1\n\t"                                                                      \
    "v_mov_b32 v44, -1\n\t"                                                                      \
    "v_mov_b32 v48, -1\n\t"                                                                      \
    "v_mov_b32 v52, -1\n\t"                                                                      \
    "v_mov_b32 v56, -1\n\t"                                                                      \
    "v_mov_b32 v60, -1\n\t"                                                                      \
    "v_mov_b32 v106, -1\n\t" /* LIVE: no job of the batch is running */
// The decision is the pick and the commit alone: a placed job takes no slot.  The commit is
// MCS_FA_DECIDE16R's chunk move in its register-index region, as a v_cndmask under the fitting lane's mask
// in s[60:61] (a temporary of the bulk move and the releases, free in a pass): the lane's chunk takes the
// difference, every other lane keeps its own, and exec stays the full wave from the fit test to the record
// read ("Fit and commit"; the zero route commits nothing, MCS_FA_ZEROKX16C).  It stays in its batch lane, its finish in the LIVE column v106
// (written beside the two result writes; -1 in every other lane), until it finishes there or the batch
// ends and the live lanes go into their calendar rows together (MCS_FC_BMOVE).
#define MCS_FA_DECIDE16C                                                                          \
    "v_readlane_b32 s51, v86, s50\n\t"                                                            \
    "s_lshl_b64 s[60:61], 1, s50\n\t" /* the fitting lane's mask (s[60:61]: free in a pass) */  \
    "s_ff1_i32_b32 s52, s51\n\t"                                                                  \
    "s_lshr_b32 s53, s52, 3\n\t"                                                                  \
    "s_lshl2_add_u32 s54, s50, s53\n\t" /* kx = the node index, lane * 4 + chunk */             \
    "s_set_gpr_idx_on s53, gpr_idx(SRC0,SRC1,DST)\n\t"                                            \
    "v_cndmask_b32_e64 v64, v64, v72, s[60:61]\n\t" /* the commit (cluster.go:146-147) */         \
    "s_set_gpr_idx_off\n\t"
// a batch-lane release (out of line; vcc = the lanes of LIVE that finish by t, not empty): the LDS node
// copy is refreshed, the requests (v96) go back to the nodes (base + 4 * v91) and the lanes leave LIVE;
// then the calendar row of the second, with its body if it expires; s76 = the count of both, and into
// the tail TAIL of the copy or of its waiting-head section.  P prefixes the labels.
#define MCS_FC_BREL(P, k, F, PAY, A, FREE, TAIL)                                                  \
    "mcsfa_" P #k "_%=:\n\t"                                                                      \
    "ds_write_b128 v108, v[64:67]\n\t"                                                           \
    "s_mov_b64 exec, vcc\n\t"                                                                     \
    "s_bcnt1_i32_b64 s76, vcc\n\t"                                                               \
    "v_lshl_add_u32 v121, v91, 2, v109\n\t"                                                      \
    "ds_add_u32 v121, v96\n\t"                                                                    \
    "v_sub_u32 v92, v106, v95\n\t" /* the start: finish - the lane's duration */                 \
    "v_mov_b32 v106, -1\n\t"                                                                      \
    "s_mov_b64 exec, -1\n\t"                                                                      \
    "v_cmp_ge_u32_e32 vcc, s40, " F "\n\t"                                                       \
    "s_cbranch_vccz mcsfa_" TAIL #k "_%=\n\t"                                                     \
    "s_mov_b64 exec, vcc\n\t"                                                                     \
    "s_bcnt1_i32_b64 s49, vcc\n\t"                                                               \
    "ds_add_u32 " A ", " PAY "\n\t"                                                             \
    "v_mov_b32 " F ", -1\n\t"                                                                    \
    "s_or_b64 " FREE ", " FREE ", vcc\n\t"                                                       \
    "s_add_u32 s76, s76, s49\n\t"                                                                 \
    "s_branch mcsfa_" TAIL #k "_%=\n"
// The bulk move at the batch end (after the result stores, before the columns are recycled): the lanes
// with LIVE != -1 go to row LIVE & 7, each row's candidates matched to its free lanes by rank.  The
// candidates are numbered row after row (v_mbcnt on the row's candidate mask, on top of the rows before:
// O[r] in s50-s55, s62, s63 is the count of rows 0 .. r) and write {finish, request, node address} to
// the 16-byte entry of their number in the LDS scratch behind the node words (base + 1024); free lane
// number j of row r reads entry O[r-1] + j while that is below O[r]: one masked ds_read_b128 per row, straight
// into the row's quad v[32+4r : 35+4r] = {finish, payload, node address, a word nothing reads} under exec = the
// lanes that take an entry, the other lanes keeping what they hold (eight reads, one wait).  A row
// with more candidates than free lanes (out of line, mcsfa_bmo<r>) marks the ones beyond in s[46:47];
// they go one at a time, as a per-job insert did, to the first row r+1 ... r+7 (mod 8) with a free lane,
// XMIN = min(XMIN, finish).  The pool cannot be short: the batch end has left on peak > 64*8, and below
// that the free slots are at least the live lanes (a row search that comes round is a pool overflow all
// the same).  Temporaries: s[46:49] (set again by the batch take), s49, s75, s76, s79, s85, s[50:55],
// s[60:63], v112-v115, v120-v123.
#define MCS_FC_BMA(r, OP, ON, FREE)                                                               \
    "v_cmp_eq_u32_e64 s[60:61], " #r ", v122\n\t"                                                 \
    "s_bcnt1_i32_b64 s76, s[60:61]\n\t"                                                           \
    "v_mbcnt_lo_u32_b32 v120, s60, v121\n\t"                                                      \
    "s_bcnt1_i32_b64 s75, " FREE "\n\t"                                                           \
    "v_mbcnt_hi_u32_b32 v120, s61, v120\n\t"                                                      \
    "s_add_u32 " ON ", " OP ", s76\n\t"                                                           \
    "v_cndmask_b32_e64 v123, v123, v120, s[60:61]\n\t"                                            \
    "s_cmp_gt_u32 s76, s75\n\t"                                                                   \
    "s_cbranch_scc1 mcsfa_bmo" #r "_%=\n"                                                         \
    "mcsfa_bmr" #r "_%=:\n\t"                                                                     \
    "v_mov_b32 v121, " ON "\n\t"
// (row r's candidates beyond its free lanes: number >= O[r-1] + the free lanes)
#define MCS_FC_BMO(r, OP)                                                                         \
    "mcsfa_bmo" #r "_%=:\n\t"                                                                     \
    "s_add_u32 s75, s75, " OP "\n\t"                                                              \
    "v_cmp_le_u32_e32 vcc, s75, v120\n\t"                                                         \
    "s_and_b64 vcc, vcc, s[60:61]\n\t"                                                            \
    "s_or_b64 s[46:47], s[46:47], vcc\n\t"                                                        \
    "s_branch mcsfa_bmr" #r "_%=\n"
#define MCS_FC_BMB(OP, ON, FREELO, FREEHI, FREE, Q)                                               \
    "v_mov_b32 v121, " OP "\n\t"                                                                  \
    "v_mbcnt_lo_u32_b32 v120, " FREELO ", v121\n\t"                                               \
    "v_mbcnt_hi_u32_b32 v120, " FREEHI ", v120\n\t"                                               \
    "v_cmp_gt_u32_e64 s[60:61], " ON ", v120\n\t"                                                 \
    "v_lshl_add_u32 v120, v120, 4, v109\n\t"                                                      \
    "s_and_b64 exec, s[60:61], " FREE "\n\t"                                                      \
    "ds_read_b128 " Q ", v120 offset:1024\n\t"                                                    \
    "s_andn2_b64 " FREE ", " FREE ", exec\n\t"                                                    \
    "s_mov_b64 exec, -1\n\t"
#define MCS_FC_BMOVE                                                                              \
    "v_cmp_ne_u32_e32 vcc, -1, v106\n\t"                                                          \
    "s_cbranch_vccz mcsfa_bmx_%=\n\t"                                                             \
    "v_and_b32 v122, 7, v106\n\t"                                                                 \
    "s_mov_b64 s[48:49], vcc\n\t" /* the live lanes */                                           \
    "v_cndmask_b32_e32 v122, 8, v122, vcc\n\t" /* the lane's row; 8: none */                     \
    "s_mov_b64 s[46:47], 0\n\t"                                                                   \
    "v_mov_b32 v112, v106\n\t"                                                                    \
    "v_mov_b32 v113, v96\n\t"                                                                     \
    "v_lshl_add_u32 v114, v91, 2, v109\n\t"                                                       \
    "v_mov_b32 v121, 0\n\t"                                                                       \
    MCS_FC_BMA(0, "0", "s50", "s[86:87]") MCS_FC_BMA(1, "s50", "s51", "s[88:89]")                 \
    MCS_FC_BMA(2, "s51", "s52", "s[90:91]") MCS_FC_BMA(3, "s52", "s53", "s[92:93]")               \
    MCS_FC_BMA(4, "s53", "s54", "s[94:95]") MCS_FC_BMA(5, "s54", "s55", "s[96:97]")               \
    MCS_FC_BMA(6, "s55", "s62", "s[98:99]") MCS_FC_BMA(7, "s62", "s63", "s[100:101]")             \
    "s_mov_b64 exec, s[48:49]\n\t"                                                                \
    "v_lshl_add_u32 v123, v123, 4, v109\n\t"                                                      \
    "ds_write_b128 v123, v[112:115] offset:1024\n\t"                                              \
    "s_mov_b64 exec, -1\n\t"                                                                      \
    MCS_FC_BMB("0", "s50", "s86", "s87", "s[86:87]", "v[32:35]")                                  \
    MCS_FC_BMB("s50", "s51", "s88", "s89", "s[88:89]", "v[36:39]")                                \
    MCS_FC_BMB("s51", "s52", "s90", "s91", "s[90:91]", "v[40:43]")                                \
    MCS_FC_BMB("s52", "s53", "s92", "s93", "s[92:93]", "v[44:47]")                                \
    MCS_FC_BMB("s53", "s54", "s94", "s95", "s[94:95]", "v[48:51]")                                \
    MCS_FC_BMB("s54", "s55", "s96", "s97", "s[96:97]", "v[52:55]")                                \
    MCS_FC_BMB("s55", "s62", "s98", "s99", "s[98:99]", "v[56:59]")                                \
    MCS_FC_BMB("s62", "s63", "s100", "s101", "s[100:101]", "v[60:63]")                            \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                    \
    "s_cmp_lg_u64 s[46:47], 0\n\t"                                                                \
    "s_cbranch_scc1 mcsfa_bml_%=\n"                                                               \
    "mcsfa_bmd_%=:\n\t"                                                                           \
    "v_mov_b32 v106, -1\n"                                                                        \
    "mcsfa_bmx_%=:\n\t"
// the out-of-line parts of the bulk move (behind the batch end's closing branch): the rows' surplus
// marks and the one-at-a-time insert of the jobs marked (s[46:47], not empty)
#define MCS_FC_BMOVE_OOL                                                                          \
    MCS_FC_BMO(0, "0") MCS_FC_BMO(1, "s50") MCS_FC_BMO(2, "s51") MCS_FC_BMO(3, "s52")             \
    MCS_FC_BMO(4, "s53") MCS_FC_BMO(5, "s54") MCS_FC_BMO(6, "s55") MCS_FC_BMO(7, "s62")           \
    "mcsfa_bml_%=:\n\t"                                                                           \
    "s_ff1_i32_b64 s52, s[46:47]\n\t"                                                             \
    "s_lshl_b64 s[60:61], 1, s52\n\t"                                                             \
    "v_readlane_b32 s55, v106, s52\n\t" /* finish */                                             \
    "v_readlane_b32 s48, v96, s52\n\t"  /* request */                                            \
    "v_readlane_b32 s54, v91, s52\n\t"  /* node */                                               \
    "s_andn2_b64 s[46:47], s[46:47], s[60:61]\n\t"                                                \
    "s_and_b32 s76, s55, 7\n\t"                                                                   \
    "s_mov_b32 s49, s76\n"                                                                        \
    "mcsfa_bms_%=:\n\t"                                                                           \
    "s_add_u32 s49, s49, 1\n\t"                                                                   \
    "s_and_b32 s49, s49, 7\n\t"                                                                   \
    "s_cmp_eq_u32 s49, s76\n\t"                                                                   \
    "s_cbranch_scc1 mcsfa_poolovf_%=\n\t"                                                         \
    "s_lshl_b32 m0, s49, 1\n\t"                                                                   \
    "s_nop 0\n\t"                                                                                 \
    "s_movrels_b64 s[60:61], s[86:87]\n\t"                                                        \
    "s_cmp_lg_u64 s[60:61], 0\n\t"                                                                \
    "s_cbranch_scc0 mcsfa_bms_%=\n\t"                                                             \
    "s_ff1_i32_b64 s85, s[60:61]\n\t"                                                             \
    "s_lshl_b64 s[62:63], 1, s85\n\t"                                                             \
    "s_andn2_b64 s[50:51], s[60:61], s[62:63]\n\t"                                                \
    "s_movreld_b64 s[86:87], s[50:51]\n\t"                                                        \
    "s_min_u32 s77, s77, s55\n\t"                                                                 \
    "s_lshl2_add_u32 s79, s54, s73\n\t"                                                           \
    "s_lshl_b32 s75, s49, 2\n\t" /* the row's quad: v(32 + 4r) */                                \
    "s_mov_b64 exec, s[62:63]\n\t"                                                                \
    "s_set_gpr_idx_on s75, gpr_idx(DST)\n\t"                                                      \
    "v_mov_b32 v32, s55\n\t"                                                                      \
    "v_mov_b32 v33, s48\n\t"                                                                      \
    "v_mov_b32 v34, s79\n\t"                                                                      \
    "s_set_gpr_idx_off\n\t"                                                                       \
    "s_mov_b64 exec, -1\n\t"                                                                      \
    "s_cmp_lg_u64 s[46:47], 0\n\t"                                                                \
    "s_cbranch_scc1 mcsfa_bml_%=\n\t"                                                             \
    "s_branch mcsfa_bmd_%=\n"
// the wave's minimum of v120 into an SGPR (MCS_FA_SCANEND's chain)
#define MCS_FC_WMIN(DST)                                                                          \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"                     \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"                     \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"                     \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"                     \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"                  \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"                  \
    "s_nop 1\n\t"                                                                                 \
    "v_readlane_b32 " DST ", v120, 63\n\t"
// the full scan's rows, one after the other (the slow path: no compare ahead of its row)
#define MCS_FC_FROW(p, F, P, A, FREE)                                                             \
    "v_cmp_ge_u32_e32 vcc, s40, " F "\n\t" /* (under the full wave) */                          \
    "s_cbranch_vccz mcsfa_fr" #p "_%=\n\t"                                                       \
    "s_mov_b64 exec, vcc\n\t"                                                                     \
    "s_bcnt1_i32_b64 s76, vcc\n\t"                                                               \
    "ds_add_u32 " A ", " P "\n\t"                                                               \
    "v_mov_b32 " F ", -1\n\t"                                                                    \
    "s_add_u32 s49, s49, s76\n\t"                                                                \
    "s_or_b64 " FREE ", " FREE ", vcc\n\t"                                                       \
    "s_mov_b64 exec, -1\n"                                                    \
    "mcsfa_fr" #p "_%=:\n\t"
// (a slot of row p counts towards XMIN when finish & 7 != p; v111 = -1)
#define MCS_FC_XROW(p, F)                                                                         \
    "v_and_b32 v121, 7, " F "\n\t"                                                               \
    "v_cmp_ne_u32_e32 vcc, " #p ", v121\n\t"                                                     \
    "v_cndmask_b32_e32 v121, v111, " F ", vcc\n\t"                                               \
    "v_min_u32 v120, v120, v121\n\t"
#define MCS_FC_FULL                                                                               \
    "mcsfa_full_%=:\n\t"                                                                          \
    "ds_write_b128 v108, v[64:67]\n\t"                                                           \
    "s_mov_b32 s49, 0\n\t"                                                                        \
    MCS_FC_FROW(0, "v32", "v33", "v34", "s[86:87]") MCS_FC_FROW(1, "v36", "v37", "v38", "s[88:89]") \
    MCS_FC_FROW(2, "v40", "v41", "v42", "s[90:91]") MCS_FC_FROW(3, "v44", "v45", "v46", "s[92:93]") \
    MCS_FC_FROW(4, "v48", "v49", "v50", "s[94:95]") MCS_FC_FROW(5, "v52", "v53", "v54", "s[96:97]") \
    MCS_FC_FROW(6, "v56", "v57", "v58", "s[98:99]") MCS_FC_FROW(7, "v60", "v61", "v62", "s[100:101]") \
    /* the ninth row: the batch lanes (LIVE), their requests back to the nodes base + 4 * v91 */  \
    "v_cmp_ge_u32_e32 vcc, s40, v106\n\t"                                                        \
    "s_cbranch_vccz mcsfa_fr8_%=\n\t"                                                            \
    "s_mov_b64 exec, vcc\n\t"                                                                    \
    "s_bcnt1_i32_b64 s76, vcc\n\t"                                                              \
    "v_lshl_add_u32 v121, v91, 2, v109\n\t"                                                     \
    "ds_add_u32 v121, v96\n\t"                                                                   \
    "v_sub_u32 v92, v106, v95\n\t" /* the start */                                               \
    "v_mov_b32 v106, -1\n\t"                                                                     \
    "s_add_u32 s49, s49, s76\n\t"                                                                \
    "s_mov_b64 exec, -1\n"                                                                       \
    "mcsfa_fr8_%=:\n\t"                                                                          \
    "s_cmp_lt_u32 s40, s77\n\t" /* no misplaced slot was due: XMIN stands */                    \
    "s_cbranch_scc1 mcsfa_fx_%=\n\t"                                                              \
    "v_mov_b32 v120, -1\n\t"                                                                      \
    MCS_FC_XROW(0, "v32") MCS_FC_XROW(1, "v36") MCS_FC_XROW(2, "v40") MCS_FC_XROW(3, "v44")      \
    MCS_FC_XROW(4, "v48") MCS_FC_XROW(5, "v52") MCS_FC_XROW(6, "v56") MCS_FC_XROW(7, "v60")      \
    MCS_FC_WMIN("s77") "\n"                                                                      \
    "mcsfa_fx_%=:\n\t"                                                                            \
    "s_mov_b32 s76, s49\n\t"                                                                      \
    "s_cmp_eq_u32 s49, 0\n\t"                                                                     \
    "s_cbranch_scc1 mcsfa_norel_%=\n\t"                                                           \
    "s_branch mcsfa_reltail_%=\n"
// every running job's earliest finish into s76, the batch lanes' (LIVE) with the slots' (lane-minimum
// tree + DPP; free slots and lanes hold -1)
#define MCS_FC_EXACTMIN                                                                           \
    "v_min3_u32 v121, v32, v36, v40\n\t"                                                         \
    "v_min3_u32 v121, v121, v44, v48\n\t"                                                        \
    "v_min3_u32 v121, v121, v52, v56\n\t"                                                        \
    "v_min3_u32 v120, v121, v60, v106\n\t" MCS_FC_WMIN("s76")
// the zero route (out of line, from mcsfa_arrive): the true arrival's test and the sleep to it, or the
// fit test and mcsfa_zero.  A zero-duration job that fits nowhere waits out of line as well
// (mcsfa_znofit, s43 = 2; 1 in 600 jobs has zero duration and few of those wait, so the copies' waiting-
// head sections know nothing of it): counted and guarded as every failed fit, then the clock jumps to
// the exact earliest finish, every row is scanned (mcsfa_full, which comes back to mcsfa_zreltail
// through the table: s43 selects the entry), and the release's bookkeeping ends in mcsfa_zfit again.
// The seconds in between have no completion, so the releases, the failed fits and both counters are
// those of a sleep taken second by second.  Placed (mcsfa_zero, which tests s43), it is counted as
// waited, the next job's record is read and the head sleeps its second (mcsfa_zhead).
#define MCS_FC_ZROUTE(D)                                                                          \
    "mcsfa_zarr_%=:\n\t"                                                                          \
    "s_cmp_eq_u32 s47, 64\n\t" /* no job left in the batch, or in the stream: the batch end */  \
    "s_cbranch_scc1 mcsfa_bend_%=\n\t"                                                            \
    "s_add_u32 s76, s57, s47\n\t"                                                                 \
    "s_cmp_ge_u32 s76, s42\n\t"                                                                   \
    "s_cbranch_scc1 mcsfa_bend_%=\n\t"                                                            \
    "v_readlane_b32 s76, v87, s47\n\t" /* the true arrival */                                    \
    "s_cmp_lg_u32 s46, 0\n\t"                                                                     \
    "s_cselect_b32 s76, s45, s76\n\t" /* (a non-zero job: the arrival it carries) */             \
    "s_cmp_gt_u32 s76, s40\n\t"                                                                   \
    "s_cbranch_scc0 mcsfa_zfit_%=\n\t"                                                            \
    "s_sub_u32 s49, s76, s40\n\t"                                                                 \
    "s_mov_b32 s40, s76\n\t" /* not arrived: sleep to it */                                      \
    MCS_FA_CNTS_##D                                                                               \
    "s_cmp_lg_u32 s49, 1\n\t"                                                                     \
    "s_cbranch_scc1 mcsfa_full_%=\n\t"                                                            \
    "s_branch mcsfa_adv1_%=\n"                                                                    \
    "mcsfa_zfit_%=:\n\t" MCS_FA_FIT16C MCS_FA_ANYFIT                                             \
    "s_cbranch_vccz mcsfa_znofit_%=\n\t"                                                          \
    "s_ff1_i32_b64 s50, vcc\n\t"                                                                  \
    "s_branch mcsfa_zero_%=\n"                                                                    \
    "mcsfa_znofit_%=:\n\t"                                                                        \
    "s_mov_b32 s43, 2\n\t"                                                                        \
    MCS_FA_CNTS_##D                                                                               \
    "s_sub_u32 s78, s78, 1\n\t" /* the runaway guard */                                          \
    "s_cbranch_scc1 mcsfa_poolovf_%=\n\t"                                                         \
    "s_cmp_eq_u32 s80, 0\n\t" /* nothing running */                                              \
    "s_cbranch_scc1 mcsfa_deadlock_%=\n\t" MCS_FC_EXACTMIN                                        \
    "s_cmp_eq_u32 s76, -1\n\t" /* (a count without a slot or a live lane: flagged) */            \
    "s_cbranch_scc1 mcsfa_poolovf_%=\n\t"                                                         \
    "s_max_u32 s40, s40, s76\n\t"                                                                 \
    "s_branch mcsfa_full_%=\n"                                                                    \
    "mcsfa_zreltail_%=:\n\t" MCS_FA_CNTR_##D                                                     \
    "s_max_u32 s81, s81, s80\n\t"                                                                 \
    "s_mov_b64 exec, -1\n\t"                                                                      \
    "s_sub_u32 s80, s80, s76\n\t" MCS_FA_RELOAD16C                                               \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                    \
    "s_branch mcsfa_zfit_%=\n"                                                                    \
    "mcsfa_zhead_%=:\n\t" /* (m0 = the head's lane, from mcsfa_zero) */                          \
    "s_add_u32 s82, s82, 1\n\t"                                                                   \
    "s_mov_b32 s43, 0\n\t" MCS_FC_RECNEXT                                                        \
    "s_add_u32 s47, s47, 1\n\t"                                                                   \
    "s_add_u32 s40, s40, 1\n\t"                                                                   \
    "s_branch mcsfa_adv1_%=\n"
// One copy of the loop per clock residue ("One loop test per pass"): the wave runs copy
// t & 7, whose row block compares its row's registers, named in the text.  Whatever advances the clock by
// one second goes on at the next copy's row block: the placed WaitQueue head's sleep falls through into it,
// an arrival one second on branches there; only the XMIN test stays at the advance.  The paths that set the clock to any second, or that all copies share (the full scan, the
// exact-minimum fallback, the batch end with its bulk move, the zero route), are single and come back through a
// table of branches, eight per entry point (MCS_FC_RET: s74 + 32 * entry + 4 * (t & 7), the table on a
// 512-byte line and 320 bytes long, so the sum never carries).  The padding in front of a copy's
// mcsfa_norel lies behind an unconditional branch and is never run; it puts the pass's head (mcsfa_fit)
// 24 bytes into a 64-byte line: 16, the position MCS_FA_HEAD16C kept for the single loop, while the fit test
// was 8 bytes longer, so what lies behind the test is where it was; again the best of the eight 4-byte
// positions at 4096 and at 512 clusters (profiles/fit_commit/ab_place_*.txt).
//
// A waiting WaitQueue head has a section of its own in each copy ("The waiting head"),
// entered at the failed fit (mcsfa_nofit<k>) and left when the head is placed; nothing else runs while
// s43 = 1.  Its sleep is a chain of eight blocks, one per residue, laid out one after the other behind the
// copies (MCS_FC_WSL): a step is the clock's s_add, one compare against the limit s79 = min(XMIN, t + 9)
// formed at the failed fit (XMIN cannot change in a sleep: nothing is inserted, and a full scan comes
// back through mcsfa_wnorel or the failed fit, which form the limit again), the row's v_cmp and the
// branch to the section's release, and falls into the next residue's block.  At the limit (mcsfa_wslow) a
// misplaced slot is due (the full scan) or eight rows have been compared for nothing (mcsfa_exact: the
// jump to the exact earliest finish).  The section's release (mcsfa_wrel<k>) is the row block's body and
// the tail without the arrival compare: the head has arrived.  A failed re-test is a failed fit again
// (the guard counts, the limit is formed again).  The head's placement is the pass's decision and
// result writes, then without a test: it is counted as waited, s43 = 0, the next job's record, the
// one-second sleep (:250), the XMIN test, and the next copy's ordinary row block.  The single paths a
// waiting head can take (the full scan) return through MCS_FC_RETW, whose table entry is
// e + s43: the waiting head's entry follows the ordinary one, a waiting zero-duration job's (s43 = 2,
// MCS_FC_ZROUTE) that one.
// The one-second advances carry no overflow branch: the host bounds last arrival + sum(dur + 1) below
// 2^32 - 1 for every stream that runs this loop (mcs_submit_jobs, mcs_generate_jobs; unchecked_horizon
// runs the compiled kernel), and no clock of the run exceeds that sum; a clock that did reach
// 0xffffffff is still flagged after the loop (fifo_asm_kernel).
// Table entries: 0 blk, 1 norel, 2 wnorel, 3 (zero job, no release: cannot be, flagged), 4 reltail,
// 5 wreltail, 6 zreltail, 7 wblk, 8 inner, 9 placed.
#define MCS_FC_RET(TMP, e)                                                                        \
    "s_and_b32 " TMP ", s40, 7\n\t"                                                               \
    "s_lshl2_add_u32 s58, " TMP ", s74\n\t"                                                       \
    "s_add_u32 s58, s58, 32*" #e "\n\t"                                                           \
    "s_setpc_b64 s[58:59]\n"
#define MCS_FC_RETW(TMP, e)                                                                       \
    "s_and_b32 " TMP ", s40, 7\n\t"                                                               \
    "s_lshl3_add_u32 " TMP ", s43, " TMP "\n\t"                                                   \
    "s_lshl2_add_u32 s58, " TMP ", s74\n\t"                                                       \
    "s_add_u32 s58, s58, 32*" #e "\n\t"                                                           \
    "s_setpc_b64 s[58:59]\n"
#define MCS_FC_TBL1(name)                                                                         \
    "s_branch mcsfa_" name "_%=\n\t"                                                              \
    "s_branch mcsfa_" name "_%=\n\t"                                                              \
    "s_branch mcsfa_" name "_%=\n\t"                                                              \
    "s_branch mcsfa_" name "_%=\n\t"                                                              \
    "s_branch mcsfa_" name "_%=\n\t"                                                              \
    "s_branch mcsfa_" name "_%=\n\t"                                                              \
    "s_branch mcsfa_" name "_%=\n\t"                                                              \
    "s_branch mcsfa_" name "_%=\n\t"
#define MCS_FC_TBL(name)                                                                          \
    "s_branch mcsfa_" name "0_%=\n\t"                                                             \
    "s_branch mcsfa_" name "1_%=\n\t"                                                             \
    "s_branch mcsfa_" name "2_%=\n\t"                                                             \
    "s_branch mcsfa_" name "3_%=\n\t"                                                             \
    "s_branch mcsfa_" name "4_%=\n\t"                                                             \
    "s_branch mcsfa_" name "5_%=\n\t"                                                             \
    "s_branch mcsfa_" name "6_%=\n\t"                                                             \
    "s_branch mcsfa_" name "7_%=\n\t"
// the XMIN test of a one-second advance into copy n: a misplaced slot due goes to the full scan
#define MCS_FC_ADV(n)                                                                             \
    "s_cmp_ge_u32 s40, s77\n\t"                                                                   \
    "s_cbranch_scc1 mcsfa_full_%=\n\t"                                                            \
    "s_branch mcsfa_blk" #n "_%=\n"
// copy k (row k: finish F, payload P, node address A, free lanes FREE), n = k + 1 mod 8; TAIL closes the
// placed head's sleep: nothing where the next copy's row block follows, a branch to copy 0 after copy 7
#define MCS_FC_COPY(D, k, n, F, P, A, FREE, TAIL)                                                 \
    /* the row against t; an expiry refreshes the LDS node copy under the full wave, then hands */ \
    /* the payloads back under exec = the expiry mask (vcc) and falls into the tail */           \
    "mcsfa_blk" #k "_%=:\n\t"                                                                     \
    "v_cmp_ge_u32_e32 vcc, s40, v106\n\t" /* the batch lanes (LIVE): a release out of line */   \
    "s_cbranch_vccnz mcsfa_brel" #k "_%=\n\t"                                                     \
    "v_cmp_ge_u32_e32 vcc, s40, " F "\n\t"                                                       \
    "s_cbranch_vccz mcsfa_norel" #k "_%=\n\t"                                                     \
    "ds_write_b128 v108, v[64:67]\n\t"                                                           \
    "s_mov_b64 exec, vcc\n\t"                                                                     \
    "s_bcnt1_i32_b64 s76, vcc\n\t"                                                               \
    "ds_add_u32 " A ", " P "\n\t"                                                               \
    "v_mov_b32 " F ", -1\n\t"                                                                    \
    "s_or_b64 " FREE ", " FREE ", vcc\n"                                                         \
    /* released (s76 slots; exec any): the peak before the count falls, the node reload, the */  \
    /* head's fit test and the arrival test.  A head that has arrived (s45 <= t) enters the pass */ \
    /* at mcsfa_fitted.  Otherwise (no job left in the batch, a zero-duration job: 0xffffffff; */  \
    /* or a later arrival) the fit test's results are dropped (temporaries only: v72-v75, v80, */  \
    /* v81, v86, vcc, s55) and the loop goes on at mcsfa_arrive.  The same instructions are */    \
    /* issued either way, so there is one tail.  (No head waits here: its section has a tail.) */      \
    "mcsfa_reltail" #k "_%=:\n\t" MCS_FA_CNTR_##D                                                \
    "s_max_u32 s81, s81, s80\n\t"                                                                 \
    "s_mov_b64 exec, -1\n\t"                                                                      \
    "s_sub_u32 s80, s80, s76\n\t" MCS_FA_RELOAD16C                                               \
    "s_add_u32 s55, s40, s46\n\t" /* finish */                                                   \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                    \
    MCS_FA_FITBITS16C("s_cmp_le_u32 s45, s40\n\t") MCS_FA_ANYFIT                                 \
    "s_cbranch_scc1 mcsfa_fitted" #k "_%=\n\t"                                                    \
    "s_branch mcsfa_arrive" #k "_%=\n"                                                            \
    ".p2align 6\n\t"                                                                              \
    "s_nop 0\n\t" /* (never run: mcsfa_fit 24 bytes into the line) */                            \
    "s_nop 0\n\t"                                                                                 \
    "s_nop 0\n\t"                                                                                 \
    "s_nop 0\n"                                                                                   \
    /* nothing released: the advance ends (a sleeping head never comes here) */                  \
    "mcsfa_norel" #k "_%=:\n"                                                                     \
    "mcsfa_inner" #k "_%=:\n\t"                                                                   \
    "s_cmp_gt_u32 s45, s40\n\t" /* ready head not arrived: sleep to it */                         \
    "s_cbranch_scc1 mcsfa_arrive" #k "_%=\n"                                                      \
    "mcsfa_fit" #k "_%=:\n\t" MCS_FA_FIT16C MCS_FA_ANYFIT "\n"                                   \
    "mcsfa_fitted" #k "_%=:\n\t" /* (a release enters here, the fit test done in its tail) */    \
    "s_cbranch_vccz mcsfa_nofit" #k "_%=\n\t"                                                     \
    "s_ff1_i32_b64 s50, vcc\n\t" /* lowest lane with a fit */                                     \
    MCS_FA_DECIDE16C                                                                              \
    "s_mov_b32 m0, s47\n\t"                                                                       \
    "s_add_u32 s80, s80, 1\n\t"                                                                   \
    "v_writelane_b32 v91, s54, m0\n\t"                                                            \
    "v_writelane_b32 v106, s55, m0\n" /* LIVE: the job runs in its batch lane */                                                              \
    /* next ready job */                                                                          \
    /* (m0 = the lane of the job just placed; no next job in the batch and a zero-duration one */ \
    /* both read as the arrival 0xffffffff: one bottom test) */                                   \
    "mcsfa_placed" #k "_%=:\n\t" MCS_FC_RECNEXT                                                  \
    "s_add_u32 s47, s47, 1\n\t"                                                                   \
    "s_cmp_le_u32 s45, s40\n\t"                                                                   \
    "s_cbranch_scc1 mcsfa_fit" #k "_%=\n\t"                                                       \
    "s_cmp_eq_u32 s45, -1\n\t"                                                                    \
    "s_cbranch_scc1 mcsfa_zarr_%=\n"                                                              \
    /* a later arrival: sleep to it; more than a second on, every row is scanned */              \
    "mcsfa_arr2" #k "_%=:\n\t"                                                                    \
    "s_sub_u32 s76, s45, s40\n\t"                                                                 \
    "s_mov_b32 s40, s45\n\t" /* (> t) */                                                         \
    MCS_FA_CNTS_##D                                                                               \
    "s_cmp_lg_u32 s76, 1\n\t"                                                                     \
    "s_cbranch_scc1 mcsfa_full_%=\n\t" MCS_FC_ADV(n)                                              \
    /* (from the pass's head and a release's tail) */                                            \
    "mcsfa_arrive" #k "_%=:\n\t"                                                                  \
    "s_cmp_eq_u32 s45, -1\n\t" /* 0xffffffff: a zero-duration job, or no job: out of line */      \
    "s_cbranch_scc1 mcsfa_zarr_%=\n\t"                                                            \
    "s_branch mcsfa_arr2" #k "_%=\n"                                                              \
    /* ---- the batch-lane releases of the row block and of the section's sleep (out of line) ---- */ \
    MCS_FC_BREL("brel", k, F, P, A, FREE, "reltail") MCS_FC_BREL("wbrel", k, F, P, A, FREE, "wreltail") \
    /* ---- the copy's waiting-head section (after the copy's text; entered by branches only) ---- */ \
    /* no node fits: the head waits (s43 = 1) and sleeps to the next completion, a second at a */ \
    /* time up to the limit s79 = min(XMIN, t + 9), in the chain of sleep blocks (MCS_FC_WSL) */   \
    "mcsfa_nofit" #k "_%=:\n\t"                                                                   \
    "s_mov_b32 s43, 1\n\t"                                                                        \
    MCS_FA_CNTS_##D                                                                               \
    "s_sub_u32 s78, s78, 1\n\t" /* the runaway guard counts down: the borrow trips it */          \
    "s_cbranch_scc1 mcsfa_poolovf_%=\n\t"                                                         \
    "s_add_u32 s79, s40, 9\n\t"                                                                   \
    "s_min_u32 s79, s79, s77\n\t"                                                                 \
    "s_cmp_eq_u32 s80, 0\n\t" /* nothing running */                                              \
    "s_cbranch_scc0 mcsfa_wsl" #n "_%=\n\t"                                                       \
    "s_branch mcsfa_deadlock_%=\n"                                                                \
    /* (a full scan at this second released nothing: the sleep goes on under a new limit) */      \
    "mcsfa_wnorel" #k "_%=:\n\t"                                                                  \
    "s_add_u32 s79, s40, 9\n\t"                                                                   \
    "s_min_u32 s79, s79, s77\n\t"                                                                 \
    "s_branch mcsfa_wsl" #n "_%=\n"                                                               \
    /* the section's release: the row block's body, and the tail for a head that has arrived */  \
    /* (vcc = the row's expiry mask; a full scan enters at mcsfa_wreltail with s76 its count) */  \
    "mcsfa_wrel" #k "_%=:\n\t"                                                                    \
    "ds_write_b128 v108, v[64:67]\n\t"                                                           \
    "s_mov_b64 exec, vcc\n\t"                                                                     \
    "s_bcnt1_i32_b64 s76, vcc\n\t"                                                               \
    "ds_add_u32 " A ", " P "\n\t"                                                               \
    "v_mov_b32 " F ", -1\n\t"                                                                    \
    "s_or_b64 " FREE ", " FREE ", vcc\n"                                                         \
    "mcsfa_wreltail" #k "_%=:\n\t" MCS_FA_CNTR_##D                                               \
    "s_max_u32 s81, s81, s80\n\t"                                                                 \
    "s_mov_b64 exec, -1\n\t"                                                                      \
    "s_sub_u32 s80, s80, s76\n\t" MCS_FA_RELOAD16C                                               \
    "s_waitcnt lgkmcnt(0)\n\t" MCS_FA_FIT16C MCS_FA_ANYFIT                                       \
    "s_cbranch_vccz mcsfa_nofit" #k "_%=\n\t" /* fails again: a failed fit like the first */     \
    /* the head's placement: the pass's decision and result writes; then it is counted as */     \
    /* waited, the next job's record is read (m0 = the head's lane), and the head sleeps a */    \
    /* second (:250) into the next copy's ordinary row block */                                  \
    "s_ff1_i32_b64 s50, vcc\n\t"                                                                  \
    MCS_FA_DECIDE16C                                                                              \
    "s_mov_b32 m0, s47\n\t"                                                                       \
    "s_add_u32 s80, s80, 1\n\t"                                                                   \
    "v_writelane_b32 v91, s54, m0\n\t"                                                            \
    "v_writelane_b32 v106, s55, m0\n\t"                                                            \
    "s_add_u32 s82, s82, 1\n\t"                                                                   \
    "s_mov_b32 s43, 0\n\t" MCS_FC_RECNEXT                                                        \
    "s_add_u32 s47, s47, 1\n\t"                                                                   \
    "s_add_u32 s40, s40, 1\n\t"                                                                   \
    "s_cmp_ge_u32 s40, s77\n\t"                                                                   \
    "s_cbranch_scc1 mcsfa_full_%=\n" TAIL
// one block of the sleep chain: the step into a second of residue k, then row k against it.  The blocks
// of the eight residues follow one another (MCS_FC_PASS), so a step that finds nothing falls into the
// next; mcsfa_wblk<k> is where the exact-minimum jump lands
#define MCS_FC_WSL(k, F)                                                                          \
    "mcsfa_wsl" #k "_%=:\n\t"                                                                     \
    "s_add_u32 s40, s40, 1\n\t"                                                                   \
    "s_cmp_ge_u32 s40, s79\n\t"                                                                   \
    "s_cbranch_scc1 mcsfa_wslow_%=\n"                                                             \
    "mcsfa_wblk" #k "_%=:\n\t"                                                                    \
    "v_cmp_ge_u32_e32 vcc, s40, v106\n\t"                                                        \
    "s_cbranch_vccnz mcsfa_wbrel" #k "_%=\n\t"                                                    \
    "v_cmp_ge_u32_e32 vcc, s40, " F "\n\t"                                                       \
    "s_cbranch_vccnz mcsfa_wrel" #k "_%=\n"
// the passes of this form (mcs_fifo_asm.hip's MCS_FA_PASS, with its own clock advances): the entry goes
// to the copy of its clock through the table, as the batch end does
#define MCS_FC_PASS(D)                                                                            \
    "s_branch mcsfa_inner_%=\n"                                                                   \
    ".p2align 6\n"                                                                                \
    MCS_FC_COPY(D, 0, 1, "v32", "v33", "v34", "s[86:87]", "")                                     \
    MCS_FC_COPY(D, 1, 2, "v36", "v37", "v38", "s[88:89]", "")                                     \
    MCS_FC_COPY(D, 2, 3, "v40", "v41", "v42", "s[90:91]", "")                                     \
    MCS_FC_COPY(D, 3, 4, "v44", "v45", "v46", "s[92:93]", "")                                     \
    MCS_FC_COPY(D, 4, 5, "v48", "v49", "v50", "s[94:95]", "")                                     \
    MCS_FC_COPY(D, 5, 6, "v52", "v53", "v54", "s[96:97]", "")                                     \
    MCS_FC_COPY(D, 6, 7, "v56", "v57", "v58", "s[98:99]", "")                                     \
    MCS_FC_COPY(D, 7, 0, "v60", "v61", "v62", "s[100:101]", "\ts_branch mcsfa_blk0_%=\n")         \
    /* ---- the sleep chain of the waiting-head sections ---- */                                 \
    MCS_FC_WSL(0, "v32") MCS_FC_WSL(1, "v36") MCS_FC_WSL(2, "v40") MCS_FC_WSL(3, "v44")           \
    MCS_FC_WSL(4, "v48") MCS_FC_WSL(5, "v52") MCS_FC_WSL(6, "v56") MCS_FC_WSL(7, "v60")           \
    "\ts_branch mcsfa_wsl0_%=\n"                                                                  \
    /* ---- the single paths ---- */                                                              \
    /* the sleep has reached its limit: a misplaced slot is due (every row is scanned), or eight */ \
    /* rows were compared for nothing and the clock jumps to the exact earliest finish */        \
    "mcsfa_wslow_%=:\n\t"                                                                         \
    "s_cmp_ge_u32 s40, s77\n\t"                                                                   \
    "s_cbranch_scc1 mcsfa_full_%=\n"                                                              \
    "mcsfa_exact_%=:\n\t" MCS_FC_EXACTMIN                                                         \
    "s_cmp_eq_u32 s76, -1\n\t" /* (a count without a slot or a live lane: flagged) */            \
    "s_cbranch_scc1 mcsfa_poolovf_%=\n\t"                                                         \
    "s_max_u32 s40, s40, s76\n\t"                                                                 \
    "s_add_u32 s79, s40, 9\n\t"                                                                   \
    "s_min_u32 s79, s79, s77\n\t"                                                                 \
    "s_cmp_ge_u32 s40, s77\n\t"                                                                   \
    "s_cbranch_scc1 mcsfa_full_%=\n\t" MCS_FC_RET("s49", 7)                                      \
    /* zero-duration job: committed and released before the next decision (D3); one that waited */ \
    /* (s43 = 2) goes on as a placed head (MCS_FC_ZROUTE) */                                      \
    "mcsfa_zero_%=:\n\t" MCS_FA_ZEROKX16C                                                        \
    "v_writelane_b32 v91, s54, m0\n\t"                                                            \
    "v_writelane_b32 v92, s40, m0\n\t"                                                            \
    "s_cmp_lg_u32 s43, 0\n\t"                                                                     \
    "s_cbranch_scc1 mcsfa_zhead_%=\n\t" MCS_FC_RET("s49", 9)                                    \
    /* the clock has moved to a second nothing but its own row's slots, or a misplaced one, can */ \
    /* have finished by (no head waits) */                                                        \
    "mcsfa_adv1_%=:\n\t"                                                                          \
    "s_cmp_ge_u32 s40, s77\n\t"                                                                   \
    "s_cbranch_scc1 mcsfa_full_%=\n\t" MCS_FC_RET("s49", 0)                                      \
    "mcsfa_norel_%=:\n\t" MCS_FC_RETW("s49", 1)                                                  \
    "mcsfa_reltail_%=:\n\t" MCS_FC_RETW("s49", 4)                                                \
    "mcsfa_inner_%=:\n\t" MCS_FC_RET("s49", 8)                                                  \
    MCS_FC_FULL MCS_FC_ZROUTE(D)                                                     \
    ".p2align 9\n"                                                                                \
    "mcsfa_tbl_%=:\n\t" MCS_FC_TBL("blk") MCS_FC_TBL("norel") MCS_FC_TBL("wnorel")               \
    MCS_FC_TBL1("poolovf") MCS_FC_TBL("reltail") MCS_FC_TBL("wreltail") MCS_FC_TBL1("zreltail") \
    MCS_FC_TBL("wblk") MCS_FC_TBL("inner") MCS_FC_TBL("placed") "\n"

// ---- W16S: W16R for clusters of at most 64 nodes (one chunk, node = lane) and 2 slot rows --------
// (cluster_small / cluster_big: C1-C3).  The fit bit is bit 15 of one SDWA AND; no chunk pick, and
// the commit is a plain move under exec = the fitting lane.  s72 = 0x7fff.
#define MCS_FA_FIT16S                                                                             \
    "v_pk_sub_u16 v72, v64, s48\n\t"                                                             \
    "v_and_b32_sdwa v80, v72, v72 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_0\n\t" \
    "v_cmp_lt_u32_e64 s[60:61], s49, v89\n\t"                                                    \
    "v_ffbl_b32 v117, v89\n\t"
#define MCS_FA_ANYFIT16S "v_cmp_lt_u32_e32 vcc, s72, v80\n\t"
#define MCS_FA_PICK116S ""
#define MCS_FA_PICK216S ""
#define MCS_FA_FREELANES16S ""
#define MCS_FA_COMMIT16S                                                                          \
    "s_mov_b32 s54, s50\n\t"                                                                     \
    "v_mov_b32 v64, v72\n\t"
#define MCS_FA_ZEROKX16S                                                                          \
    "s_mov_b32 m0, s47\n\t"                                                                      \
    "s_mov_b32 s54, s50\n\t"
#define MCS_FA_POOLMAX16S "64*2"
#define MCS_FA_NODEIDX16S "v_mov_b32 v126, v91\n\t"
#define MCS_FA_REC16S MCS_FA_REC16
#define MCS_FA_TAKE16S MCS_FA_TAKE16
#define MCS_FA_RELOAD16S "ds_read_b32 v64, v108 offset:0\n\t"
#define MCS_FA_INIT16S                                                                            \
    "s_mov_b32 s49, 0x100\n\t"                                                                   \
    "v_mov_b32 v32, -1\n\t"                                                                      \
    "v_mov_b32 v33, -1\n\t"
#define MCS_FA_INSERT16S MCS_FA_INSERT16R
#define MCS_FA_SCAN16S                                                                            \
    "ds_write_b32 v108, v64 offset:0\n\t"                                                        \
    "s_mov_b32 s75, 0\n\t"                                                                       \
    "v_cmp_ge_u32_e64 s[50:51], s40, v32\n\t"                                                    \
    "v_cmp_ge_u32_e64 s[52:53], s40, v33\n\t"                                                    \
    MCS_FR_ROW(0, "s[50:51]", "v32", "v40", "v48") MCS_FR_ROW(1, "s[52:53]", "v33", "v41", "v49")  \
    "s_mov_b64 exec, -1\n\t"                                                                     \
    "s_sub_u32 s80, s80, s75\n\t" MCS_FA_RELOAD16S                                              \
    "v_min_u32 v90, v32, v33\n\t"

// the end of a release scan: the wave's earliest remaining finish (DPP minimum of v90) under the
// node reload's latency, then the reload's wait
#define MCS_FA_SCANEND                                                                            \
    "v_mov_b32 v120, v90\n\t"                                                                     \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"                     \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"                     \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"                     \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"                     \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"                  \
    "s_nop 1\n\t"                                                                                 \
    "v_min_u32_dpp v120, v120, v120 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"                  \
    "s_nop 1\n\t"                                                                                 \
    "v_readlane_b32 s77, v120, 63\n\t"                                                            \
    "s_waitcnt lgkmcnt(0)\n\t"

// ---- MCS_STAMPS probe build (tools/stamp_fa.py): s_memtime cycles per loop segment ------------------
// s[92:93] segment start, s94 releases, s95 failed fits, s96 batch ends, s97 the whole loop; each
// stamp waits for its own SMEM read (lgkmcnt, which also drains LDS): read the shares, not the time.
// The forms built on MCS_FA_PASS carry the stamps: W32, W16, W16S and the fused W16R / W16S loops (the
// streamed three report them, mcs_debug_fa_stamps).  The streamed W16R loop (W16C) has none, because its
// FREE rows occupy s92-s101: a probe build does not contain it and runs its shape on W16.
#ifdef MCS_STAMPS
#define MCS_FA_T0 "s_memtime s[92:93]\n\ts_waitcnt lgkmcnt(0)\n\t"
#define MCS_FA_T1(acc)                                                                            \
    "s_memtime s[98:99]\n\ts_waitcnt lgkmcnt(0)\n\ts_sub_u32 s98, s98, s92\n\ts_add_u32 " acc ", " acc \
    ", s98\n\t"
#define MCS_FA_TSTART MCS_FA_T0 "s_sub_u32 s97, 0, s92\n\ts_mov_b32 s94, 0\n\ts_mov_b32 s95, 0\n\ts_mov_b32 s96, 0\n\t"
#define MCS_FA_TEND                                                                               \
    "s_memtime s[98:99]\n\ts_waitcnt lgkmcnt(0)\n\ts_add_u32 s97, s97, s98\n\t"                  \
    "s_mov_b32 %[st0], s94\n\ts_mov_b32 %[st1], s95\n\ts_mov_b32 %[st2], s96\n\ts_mov_b32 %[st3], s97\n\t"
#define MCS_FA_STAMP_CLOBBERS , "s92", "s93", "s94", "s95", "s96", "s97", "s98", "s99"
#define MCS_FA_STAMP_OUTS , [st0] "=s"(st0), [st1] "=s"(st1), [st2] "=s"(st2), [st3] "=s"(st3)
#else
#define MCS_FA_T0 ""
#define MCS_FA_T1(acc) ""
#define MCS_FA_TSTART ""
#define MCS_FA_TEND ""
#define MCS_FA_STAMP_CLOBBERS
#define MCS_FA_STAMP_OUTS
#endif

// diagnostic counters (passes without a decision, release scans): DIAG launches only
#define MCS_FA_CNTS_D1 "s_add_u32 s83, s83, 1\n\t"
#define MCS_FA_CNTR_D1 "s_add_u32 s84, s84, 1\n\t"
#define MCS_FA_CNTS_D0 ""
#define MCS_FA_CNTR_D0 ""
