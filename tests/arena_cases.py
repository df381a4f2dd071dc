"""The arena's layout (madigan_amd/csrc/mgn_arena.h), pinned row by row for
tests/test_arena_layout.py.  A state blob is a raw image of the arena, so these
offsets are part of the blob's format.

A row is (name, configuration as tests/arena_main.cpp reads it, the line it
prints): the total, every pointer of the handle as its byte offset from the
arena's base (null where the configuration has no such buffer), the views'
dimensions.  The lines were recorded from the hand-written layout this table
replaced (struct Offsets, plan() and the pointer assignments of mgn_create,
copied into a stand-alone program), and each total was checked against that
library's mgn_arena_bytes.  The shapes are those at which a layout can go
wrong: every buffer below the 256-byte rounding, odd counts, per-asset
rewards (D = A), a replay shape with F != A, the largest n-step, and the
configurations whose aux / nstep_ring are null but keep a zero-length slot."""

ROWS = [
    ("rounding_only", "N=1 A=1 W=0 nstep=1",
     "total=11264 v.ledger=0 v.mean_entry=256 v.borrowed=512 v.prices=768 v.sine_x=1024 v.ou_mean=1280 "
     "v.trend_dy=1536 v.trend_len=1792 v.trend_flags=2048 v.cash=2304 v.timestamp=2560 v.draw_skip=2816 "
     "v.shaper_a=3072 v.shaper_b=3328 v.ep_stats=3584 v.episode_stats=3840 v.ext_prices=4096 v.units=4352 "
     "v.asset_idx=4608 v.ring=null v.ring_ts=null v.ring_head=4864 v.ring_len=5120 v.win_price=null "
     "v.win_port=null v.win_ts=null v.reset_mask=5376 v.out.reward=5632 v.out.agent_reward=5888 "
     "v.out.shaped=6144 v.out.done=6400 v.out.obs_price=6656 v.out.obs_port=6912 v.out.timestamp=7168 "
     "v.out.tprice=7424 v.out.tunits=7680 v.out.tcost=7936 v.out.risk=8192 v.out.margin_call=8448 "
     "v.out.n_shaped=8704 v.out.data_end=8960 v.nstep_ring=null v.nstep_len=9216 v.nstep_head=9472 "
     "disc=9728 src=9984 target=10752 v.replay_cursor=11008 v.aux=null v.n_envs=1 v.n_assets=1 v.window=0 "
     "v.reward_dim=1 v.nstep=1 v.n_feats=1"),
    ("n3_a3", "N=3 A=3 W=0 nstep=1",
     "total=12288 v.ledger=0 v.mean_entry=256 v.borrowed=512 v.prices=768 v.sine_x=1024 v.ou_mean=1280 "
     "v.trend_dy=1536 v.trend_len=1792 v.trend_flags=2048 v.cash=2304 v.timestamp=2560 v.draw_skip=2816 "
     "v.shaper_a=3072 v.shaper_b=3328 v.ep_stats=3584 v.episode_stats=3840 v.ext_prices=4096 v.units=4352 "
     "v.asset_idx=4608 v.ring=null v.ring_ts=null v.ring_head=4864 v.ring_len=5120 v.win_price=null "
     "v.win_port=null v.win_ts=null v.reset_mask=5376 v.out.reward=5632 v.out.agent_reward=5888 "
     "v.out.shaped=6144 v.out.done=6400 v.out.obs_price=6656 v.out.obs_port=6912 v.out.timestamp=7168 "
     "v.out.tprice=7424 v.out.tunits=7680 v.out.tcost=7936 v.out.risk=8192 v.out.margin_call=8448 "
     "v.out.n_shaped=8704 v.out.data_end=8960 v.nstep_ring=null v.nstep_len=9216 v.nstep_head=9472 "
     "disc=9728 src=9984 target=11776 v.replay_cursor=12032 v.aux=null v.n_envs=3 v.n_assets=3 v.window=0 "
     "v.reward_dim=1 v.nstep=1 v.n_feats=3"),
    ("per_asset_aux_nstep3", "N=33 A=5 W=4 nstep=3 mode=2 aux=1",
     "total=104704 v.ledger=0 v.mean_entry=1536 v.borrowed=3072 v.prices=4608 v.sine_x=6144 v.ou_mean=7680 "
     "v.trend_dy=9216 v.trend_len=10752 v.trend_flags=11520 v.cash=11776 v.timestamp=12288 "
     "v.draw_skip=12800 v.shaper_a=13312 v.shaper_b=14848 v.ep_stats=16384 v.episode_stats=17152 "
     "v.ext_prices=18432 v.units=19968 v.asset_idx=21504 v.ring=21760 v.ring_ts=33536 v.ring_head=34816 "
     "v.ring_len=35072 v.win_price=35328 v.win_port=40704 v.win_ts=47104 v.reset_mask=48384 "
     "v.out.reward=48640 v.out.agent_reward=49152 v.out.shaped=50688 v.out.done=54784 "
     "v.out.obs_price=55040 v.out.obs_port=56576 v.out.timestamp=58368 v.out.tprice=58880 "
     "v.out.tunits=60416 v.out.tcost=61952 v.out.risk=63488 v.out.margin_call=63744 v.out.n_shaped=64000 "
     "v.out.data_end=64256 v.nstep_ring=64512 v.nstep_len=68608 v.nstep_head=68864 disc=69120 src=69376 "
     "target=72192 v.replay_cursor=72448 v.aux=72960 v.n_envs=33 v.n_assets=5 v.window=4 v.reward_dim=5 "
     "v.nstep=3 v.n_feats=5"),
    ("replay_feats7", "N=5 A=3 W=2 nstep=1 feats=7",
     "total=15360 v.ledger=0 v.mean_entry=256 v.borrowed=512 v.prices=768 v.sine_x=1024 v.ou_mean=1280 "
     "v.trend_dy=1536 v.trend_len=1792 v.trend_flags=2048 v.cash=2304 v.timestamp=2560 v.draw_skip=2816 "
     "v.shaper_a=3072 v.shaper_b=3328 v.ep_stats=3584 v.episode_stats=3840 v.ext_prices=4096 v.units=4352 "
     "v.asset_idx=4608 v.ring=4864 v.ring_ts=5888 v.ring_head=6144 v.ring_len=6400 v.win_price=6656 "
     "v.win_port=7424 v.win_ts=7936 v.reset_mask=8192 v.out.reward=8448 v.out.agent_reward=8704 "
     "v.out.shaped=8960 v.out.done=9216 v.out.obs_price=9472 v.out.obs_port=9984 v.out.timestamp=10240 "
     "v.out.tprice=10496 v.out.tunits=10752 v.out.tcost=11008 v.out.risk=11264 v.out.margin_call=11520 "
     "v.out.n_shaped=11776 v.out.data_end=12032 v.nstep_ring=null v.nstep_len=12288 v.nstep_head=12544 "
     "disc=12800 src=13056 target=14848 v.replay_cursor=15104 v.aux=null v.n_envs=5 v.n_assets=3 "
     "v.window=2 v.reward_dim=1 v.nstep=1 v.n_feats=7"),
    ("large_nstep256", "N=1024 A=64 W=64 nstep=256",
     "total=148437248 v.ledger=0 v.mean_entry=524288 v.borrowed=1048576 v.prices=1572864 v.sine_x=2097152 "
     "v.ou_mean=2621440 v.trend_dy=3145728 v.trend_len=3670016 v.trend_flags=3932160 v.cash=3997696 "
     "v.timestamp=4005888 v.draw_skip=4014080 v.shaper_a=4022272 v.shaper_b=4030464 v.ep_stats=4038656 "
     "v.episode_stats=4055040 v.ext_prices=4087808 v.units=4612096 v.asset_idx=5136384 v.ring=5140480 "
     "v.ring_ts=72773632 v.ring_head=73297920 v.ring_len=73302016 v.win_price=73306112 "
     "v.win_port=106860544 v.win_ts=140939264 v.reset_mask=141463552 v.out.reward=141464576 "
     "v.out.agent_reward=141472768 v.out.shaped=141480960 v.out.done=143578112 v.out.obs_price=143579136 "
     "v.out.obs_port=144103424 v.out.timestamp=144635904 v.out.tprice=144644096 v.out.tunits=145168384 "
     "v.out.tcost=145692672 v.out.risk=146216960 v.out.margin_call=146282496 v.out.n_shaped=146283520 "
     "v.out.data_end=146284544 v.nstep_ring=146285568 v.nstep_len=148382720 v.nstep_head=148386816 "
     "disc=148390912 src=148395008 target=148428288 v.replay_cursor=148429056 v.aux=null v.n_envs=1024 "
     "v.n_assets=64 v.window=64 v.reward_dim=1 v.nstep=256 v.n_feats=64"),
    ("aux0", "N=33 A=5 W=4 nstep=3 mode=2 aux=0",
     "total=72960 v.ledger=0 v.mean_entry=1536 v.borrowed=3072 v.prices=4608 v.sine_x=6144 v.ou_mean=7680 "
     "v.trend_dy=9216 v.trend_len=10752 v.trend_flags=11520 v.cash=11776 v.timestamp=12288 "
     "v.draw_skip=12800 v.shaper_a=13312 v.shaper_b=14848 v.ep_stats=16384 v.episode_stats=17152 "
     "v.ext_prices=18432 v.units=19968 v.asset_idx=21504 v.ring=21760 v.ring_ts=33536 v.ring_head=34816 "
     "v.ring_len=35072 v.win_price=35328 v.win_port=40704 v.win_ts=47104 v.reset_mask=48384 "
     "v.out.reward=48640 v.out.agent_reward=49152 v.out.shaped=50688 v.out.done=54784 "
     "v.out.obs_price=55040 v.out.obs_port=56576 v.out.timestamp=58368 v.out.tprice=58880 "
     "v.out.tunits=60416 v.out.tcost=61952 v.out.risk=63488 v.out.margin_call=63744 v.out.n_shaped=64000 "
     "v.out.data_end=64256 v.nstep_ring=64512 v.nstep_len=68608 v.nstep_head=68864 disc=69120 src=69376 "
     "target=72192 v.replay_cursor=72448 v.aux=null v.n_envs=33 v.n_assets=5 v.window=4 v.reward_dim=5 "
     "v.nstep=3 v.n_feats=5"),
    ("nstep1", "N=33 A=5 W=4 nstep=1 mode=2 aux=1",
     "total=98048 v.ledger=0 v.mean_entry=1536 v.borrowed=3072 v.prices=4608 v.sine_x=6144 v.ou_mean=7680 "
     "v.trend_dy=9216 v.trend_len=10752 v.trend_flags=11520 v.cash=11776 v.timestamp=12288 "
     "v.draw_skip=12800 v.shaper_a=13312 v.shaper_b=14848 v.ep_stats=16384 v.episode_stats=17152 "
     "v.ext_prices=18432 v.units=19968 v.asset_idx=21504 v.ring=21760 v.ring_ts=33536 v.ring_head=34816 "
     "v.ring_len=35072 v.win_price=35328 v.win_port=40704 v.win_ts=47104 v.reset_mask=48384 "
     "v.out.reward=48640 v.out.agent_reward=49152 v.out.shaped=50688 v.out.done=52224 "
     "v.out.obs_price=52480 v.out.obs_port=54016 v.out.timestamp=55808 v.out.tprice=56320 "
     "v.out.tunits=57856 v.out.tcost=59392 v.out.risk=60928 v.out.margin_call=61184 v.out.n_shaped=61440 "
     "v.out.data_end=61696 v.nstep_ring=null v.nstep_len=61952 v.nstep_head=62208 disc=62464 src=62720 "
     "target=65536 v.replay_cursor=65792 v.aux=66304 v.n_envs=33 v.n_assets=5 v.window=4 v.reward_dim=5 "
     "v.nstep=1 v.n_feats=5"),
]
