"""MI355X-native blind-bid Bulletproofs engine: thin ctypes binding over libbbp_hip.so (include/bbp.h).

The library has no CPU compute path: importing works anywhere (so the C-ABI surface can be inspected), but
`Context()` raises unless a gfx950 device is present, and the import itself raises if the HIP library was not built.
"""
from ._native import (Context, Pool, BbpError, lib, lib_path, STATUS, SIGNATURES, record_size, entropy_size,
                      LAYOUT_BLIND_G_H, LAYOUT_BLIND_G, BASE_BBLIND, BASE_G0, BASE_H0, BASE_B, NUM_BASES, STREAM_CONTEXT,
                      compile_circuit, ENTROPY_PROVE, ENTROPY_VERIFY, ENTROPY_SOURCE_OS, ENTROPY_SOURCE_DEVICE, ENTROPY_SOURCE_HEDGED, BLINDING_DRAW_MERLIN, BLINDING_DRAW_EXPANDED, prove_row_size, verify_row_size,
                      mixed_row_offsets, pack_mixed_rows, round_row_size, round_table_offsets, pack_rounds, expand_round_rows, pack_round_bids,
                      ROUND_BID_BYTES, TABLE_GENS, TABLE_PTABLE, TABLE_COMB, TABLE_BTAB, TABLE_IDX_AI, TABLE_IDX_AO, TABLE_IDX_S1,
                      TABLE_IDX_IPA, TABLE_IDX_VER, VARBASE_LANES, VARBASE_PREP_SUM, VARBASE_MX_LANES, VARBASE_MX_PREP_SUM,
                      varbase_points, SELECT_MAX_BIDS, RoundSelection, select_floor, ROW_SKIPPED, BEST_TRANCHE_DEFAULT, RoundBest, ROW_DUPLICATE, RoundBestDistinct,
                      BEST_MAX_ROUNDS, RoundsBest, RoundsBestDistinct, rounds_floors, STANDING_MAX_K, STANDING_MAX_OPEN, StandingOffer, StandingEntries, StandingsOffer)

__all__ = ["Context", "Pool", "BbpError", "lib", "lib_path", "STATUS", "SIGNATURES", "record_size", "entropy_size",
           "LAYOUT_BLIND_G_H", "LAYOUT_BLIND_G", "BASE_BBLIND", "BASE_G0", "BASE_H0", "BASE_B", "NUM_BASES", "STREAM_CONTEXT", "compile_circuit",
           "ENTROPY_PROVE", "ENTROPY_VERIFY", "ENTROPY_SOURCE_OS", "ENTROPY_SOURCE_DEVICE", "ENTROPY_SOURCE_HEDGED", "BLINDING_DRAW_MERLIN", "BLINDING_DRAW_EXPANDED", "prove_row_size", "verify_row_size", "mixed_row_offsets",
           "pack_mixed_rows", "round_row_size", "round_table_offsets", "pack_rounds", "expand_round_rows", "pack_round_bids", "ROUND_BID_BYTES",
           "TABLE_GENS", "TABLE_PTABLE", "TABLE_COMB", "TABLE_BTAB", "TABLE_IDX_AI", "TABLE_IDX_AO", "TABLE_IDX_S1", "TABLE_IDX_IPA",
           "TABLE_IDX_VER", "VARBASE_LANES", "VARBASE_PREP_SUM", "VARBASE_MX_LANES", "VARBASE_MX_PREP_SUM", "varbase_points",
           "SELECT_MAX_BIDS", "RoundSelection", "select_floor", "ROW_SKIPPED", "BEST_TRANCHE_DEFAULT", "RoundBest", "ROW_DUPLICATE",
           "RoundBestDistinct", "BEST_MAX_ROUNDS", "RoundsBest", "RoundsBestDistinct", "rounds_floors",
           "STANDING_MAX_K", "STANDING_MAX_OPEN", "StandingOffer", "StandingEntries", "StandingsOffer"]
