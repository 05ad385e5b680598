"""compute-war_amd: MI355X-native back end for compute-war's per-block hash + compress hot path.

The product is ``libcwhc.so`` (hand-written HIP kernels for gfx950 behind the C ABI declared in
``include/cw_hashcompress.h``).  This package is the thin host-side mirror of the reference's operator
interface (``doHashing`` / ``doCompression`` slots, ``HashOffload``) over that ABI via ctypes.
There is no CPU fallback: without the built library and a gfx950 device every compute call raises.
"""
from ._lib import (COMP_LZ4, COMP_LZF, COMP_NONE, HASH_NONE, HASH_SHA256, HASH_SKEIN256_128, HASH_SKEIN512,
                   CwError, lib, lib_path)
from .ops import (ACCOUNT_DTYPE, COMPOSE_DTYPE, DELTA_OP_DTYPE, PATCH_DTYPE, CdcParams, ChunkLoc, ComposeStats, DedupeIndex,
                  DeltaOp, HashOffload, IngestStats, PatchStats, ResyncWindow, ScrubStats, Store, StreamAccount, cdc_hash,
                  chunk_slot_offset, chunk_slots_bytes, compress_blocks, compress_bound, decompress_blocks, dev_apply_delta,
                  dev_cdc, dev_cdc_resync, dev_cdc_resync_windows, dev_cdc_streams, dev_cdc_streams_part, dev_compress,
                  dev_compress_chunks, dev_decompress, dev_decompress_chunks, dev_gen_mixed, dev_gen_random, dev_hash,
                  dev_hash_and_compress, dev_hash_chunks, dev_hash_tree, dev_ingest_commit, dev_ingest_commit_streams, dev_pack,
                  dev_pack_chunks, dev_read_ranges, dev_recipe_diff, dev_restore_chunks, dev_scatter_extents, dev_store_account,
                  dev_store_chunks, dev_store_compact, dev_store_export_chunks, dev_store_guard2_check, dev_store_guard2_locate,
                  dev_store_guard2_rebuild, dev_store_guard2_update, dev_store_guard_check, dev_store_guard_locate,
                  dev_store_guard_rebuild, dev_store_guard_update, dev_store_import_chunks, dev_store_mark, dev_store_renumber,
                  dev_store_replace_chunks, dev_store_verify, dev_sum_sizes, dev_translate_refs, device_count, digest_bytes,
                  do_compression, do_decompression, do_hashing, get_device, hash_and_compress_blocks, hash_and_compress_packed,
                  hash_blocks, hash_plan_describe, hash_tree_blocks, init, plan_describe, profile_enable, profile_kernels,
                  profile_read, set_block_size, set_device, shutdown, store_compose, store_guard_bytes, store_ingest,
                  store_ingest_streams, store_patch, store_restore, store_scrub, tune_reset, tune_set, tuned)
from .store import DIFF_TOTALS, LOC_DTYPE, Account, Bundle, ChunkStore, Delta, Diff, GuardSuspects, Recipe, ScrubReport, apply_delta

# (the import above also binds the submodule ``store``, which is not an export; ``ops`` has always been listed)
__all__ = [n for n in dir() if not n.startswith("_") and n != "store"]
